"""Pin of the conf layer: every conf the reference ships parses through neat_amd/conf.py, builds the HIP
model class, and `synth.ABC_NEAT_A_MODEL_CONF / _LOSS_CONF` -- which every golden fixture and bench.py call "the abc-neat-a model" --
equal the `model` / `loss` blocks of the reference's own confs/abc-neat-a.conf key for key.  A silent drift of either would
invalidate every "this is abc-neat-a" claim.  The confs are stored as parsed values in tests/golden/reference_confs.json
(tests/golden/make_conf_fixture.py); each is rendered back to conf text here and parsed again."""
import json
import os

import pytest

from neat_amd import conf as C
from neat_amd import synth

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_confs.json")
with open(FIXTURE) as _f:
    SHIPPED = json.load(_f)


def _plain(node):
    if isinstance(node, dict):
        return {k: _plain(v) for k, v in node.items()}
    if isinstance(node, (list, tuple)):
        return [_plain(v) for v in node]
    if isinstance(node, bool) or node is None or isinstance(node, str):
        return node
    return float(node)


def _render(node, indent=""):
    """A parsed tree as conf text: nested `name { ... }` blocks, `key = value`, lists, quoted strings."""
    if isinstance(node, dict):
        inner = indent + "    "
        return "{\n" + "".join(f"{inner}{k} = {_render(v, inner)}\n" for k, v in node.items()) + indent + "}"
    if isinstance(node, list):
        return "[" + ", ".join(_render(v, indent) for v in node) + "]"
    if isinstance(node, bool):
        return "true" if node else "false"
    if node is None:
        return "null"
    if isinstance(node, str):
        return json.dumps(node)
    return repr(node)


def _parse(path):
    text = f"# {path}\n" + "\n".join(f"{k} {_render(v)}" for k, v in SHIPPED[path].items())
    return C.parse_string(text)


def test_all_shipped_confs_are_found():
    assert len(SHIPPED) == 8 and "abc-neat-a.conf" in SHIPPED


@pytest.mark.parametrize("path", sorted(SHIPPED), ids=lambda p: os.path.basename(p))
def test_shipped_conf_parses_and_builds_the_model(path):
    from neat_amd import networks
    from neat_amd.loss import VolSDFLoss
    tree = _parse(path)
    assert _plain(tree) == _plain(SHIPPED[path]), path
    for block in ("train", "dataset", "model", "loss"):
        assert isinstance(tree.get_config(block), C.ConfTree), (path, block)
    # the accessors the reference's trainer and model constructor use (volsdf_train.py:141-182, rend_a :258-315)
    for key in ("train.dataset_class", "train.model_class", "train.loss_class"):
        assert "." in tree.get_string(key)
    assert tree.get_float("train.learning_rate") > 0 and tree.get_int("train.num_pixels") > 0
    model = tree.get_config("model")
    assert model.get_list("implicit_network.dims") == [256] * 8 and model.get_list("implicit_network.skip_in") == [4]
    assert model.get_int("ray_sampler.N_samples") == 64 and model.get_int("ray_sampler.max_total_iters") == 5
    m = networks.VolSDFNetwork(conf=model)                       # no conf key of any shipped file is refused
    assert sum(p.numel() for p in m.parameters() if p is not m.latents) == 1219274 - 64 * 256
    assert m.latents.shape == (model.get_int("global_junctions.num_junctions"), 256)
    assert "hip_precision" not in model and m.handle().precision == 4      # the conf names no build: the default, fp16x3
    VolSDFLoss(**dict(tree.get_config("loss").items()))


def test_synth_conf_is_the_reference_abc_neat_a_conf():
    tree = _parse("abc-neat-a.conf")
    assert _plain(tree.get_config("model")) == _plain(synth.ABC_NEAT_A_MODEL_CONF)
    assert _plain(tree.get_config("loss")) == _plain(synth.ABC_NEAT_A_LOSS_CONF)
