"""The measured-error table of the float64 kernel tests (tests/test_f64_edges.py, tests/test_f64_junction_edges.py): every comparison
records (build, entry point, size, error); NEAT_F64_TABLE=<path> appends the rows of a module as JSON lines when the module is done."""
import json
import os

import pytest
import torch

_TABLE = []


def record(build, entry, P, err):
    _TABLE.append({"build": build, "entry": entry, "P": P, "err": float(err)})
    return err


def flush():
    path = os.environ.get("NEAT_F64_TABLE")
    if path and _TABLE:
        with open(path, "a") as f:
            for row in _TABLE:
                f.write(json.dumps(row) + "\n")
    del _TABLE[:]


@pytest.fixture(scope="module", autouse=True)
def write_table():
    """Import into a test module: its rows are written once the module's last test has run."""
    yield
    flush()


def rel_err(a, b):
    """max |a - b| relative to max(1, max |b|) (test_gpu_parity.close's measure); a may live on the GPU, b is float64."""
    a = a.detach().cpu().to(torch.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all(), "non-finite values"
    if a.numel() == 0:
        return 0.0
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def check(build, entry, P, a, b, bar):
    err = record(build, entry, P, rel_err(a, b))
    assert err <= bar, f"{build} {entry} P={P}: err {err:.3e} > {bar:.1e}"
