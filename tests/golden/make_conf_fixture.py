"""Data fixture for tests/test_reference_confs.py: the eight confs the reference ships (code/confs/*.conf and
code/confs/abc/*.conf), each parsed by neat_amd/conf.py, stored as plain JSON values.

    python tests/golden/make_conf_fixture.py <reference>/code/confs

writes tests/golden/reference_confs.json: {path relative to the confs directory: parsed tree}.  Only the parsed values are
stored (no comments, no layout): the test checks the conf layer and the abc-neat-a constants of neat_amd/synth.py against
them, and re-renders each tree as conf text to run it through the parser again."""
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from neat_amd import conf as C  # noqa: E402


def _plain(node):
    if isinstance(node, dict):
        return {k: _plain(v) for k, v in node.items()}
    if isinstance(node, (list, tuple)):
        return [_plain(v) for v in node]
    return node


def main(conf_dir):
    paths = sorted(glob.glob(os.path.join(conf_dir, "*.conf")) + glob.glob(os.path.join(conf_dir, "*", "*.conf")))
    out = {os.path.relpath(p, conf_dir): _plain(C.parse_file(p)) for p in paths}
    with open(os.path.join(HERE, "reference_confs.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(out)} confs")


if __name__ == "__main__":
    main(sys.argv[1])
