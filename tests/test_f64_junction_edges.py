"""The kernels of neat_amd/csrc/kernels_junction.hpp (camera glue, projections, both line losses, the junction MLP, DBSCAN, the loss
tail, the junction gate, Adam) against float64 (tests/junction_f64.py) at the sizes where they change path: the 32-row / 16-row / 2-row
tiles of the MFMA layers and the fused kernels past 4096 rows (both settings of tuning key 28), one and several trips of the
1024-thread loss loops, the two modes of dbscan_finish_kernel (n = 5461 | 5462), the 2048-pair limit of the gate, and the aligned /
misaligned / straddling paths of adam_flat_kernel.

No test excludes elements.  A float32 kernel and a float64 reference may take different sides of a branch, so the inputs keep a margin
from every branch (relu masks, the gates, straight-or-flipped, sign(d), the matching, |cam_z| and <d, n>), and each test asserts that
margin from the float64 reference alone before it compares.  Exact zeros are put in where both sides agree exactly.

Measured on MI355X against float64, worst over every size and case below; `kernel` is the HIP kernel, `float32 CPU` the same oracle
formulation run in float32 on the CPU on the same inputs (what float32 arithmetic of the formula costs).  Values: max |a - b| / max(1,
max |b|) (tests.f64_table.rel_err); gradients and Adam's moments: max |a - b| / max |b| per tensor (junction_f64.rel_max).

    quantity                                          kernel     float32 CPU   bar
    ffn forward (y, h1, h2; both keys, J <= 4097)     3.9e-7     4.1e-7        1.5e-6
    ffn backward (dx, dW, db; ABI and autograd)       8.0e-7     1.2e-6        3e-6
    line_loss / line_losses: losses, per-line error   1.0e-7     1.0e-7        4e-7
    line_loss / line_losses: d pred                   1.4e-7     1.4e-7        6e-7
    loss_tail: scalars of scal and line3              6.9e-8     8.6e-8        3e-7
    loss_tail: gradients (rgb, grad_theta, glo3,      2.7e-7     2.7e-7        1e-6
      glo2c, pred_calib, lines3d)
    project2d, project2d_pair (|cam_z| >= 0.1)        1.7e-6     1.7e-6        7e-6
    project2d backward                                5.0e-6     5.2e-6        2e-5
    project2d, guarded depth                          7.5e-8     7.5e-8        7e-6
    l3d_points (|<d, n>| >= 0.05)                     3.7e-7     2.8e-7        1.5e-6
    inv_small (n = 1 .. 4, with row exchanges)        7.0e-8     1.1e-7        3e-7
    camera_setup: dirs, w2c (origins, K3: exact)      2.1e-7     2.1e-7        8e-7
    junction_cost                                     9.4e-8     8.2e-8        4e-7
    dbscan centres (both modes)                       1.4e-7     8.6e-7        5e-7
    Adam parameters after 1, 2, 10 steps              2.4e-7     2.4e-7        1e-6
    Adam exp_avg / exp_avg_sq                         1.0e-6     2.3e-7        2e-6

No kernel is more than 4.4x off the float32 CPU formulation (Adam's exp_avg on one-element tensors, where beta1 m + (1 - beta1) g
cancels and the kernel's fused multiply-add rounds differently); line_losses' d_pred_calib measured 6.2e-8 = one float32 rounding where
the CPU formulation happened to round to the float64 value.  junction_gate and the DBSCAN clusters are compared exactly.  Every bar is
~4x the kernel's measurement (2x for Adam's moments, whose measure is new) and below the bar of the same quantity in
test_gpu_parity.py / test_lsap.py (project2d 1e-5 / 1e-4, line loss 1e-5, ffn 1e-5 / 2e-5, Adam 2e-6, DBSCAN 1e-6).
NEAT_F64_TABLE=<path> writes every measured error as JSON lines (kernel | oracle32, entry point, size, error).
"""
import ctypes
import math
import types
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from tests import junction_f64 as jf
from tests.f64_table import record, rel_err, write_table  # noqa: F401  (write_table: the NEAT_F64_TABLE writer, autouse)
from tests.junction_f64 import F64, cached, rel_max

pytestmark = pytest.mark.gpu
POISON = -777.25

# Bars (the table above): ~4x the largest error measured on MI355X, never above the bar of the same quantity in test_gpu_parity.py /
# test_lsap.py.  Values: tests.f64_table.rel_err; gradients and moments: junction_f64.rel_max, which is never the smaller of the two.
BARS = {
    "ffn_forward": 1.5e-6, "ffn_backward": 3e-6,
    "line_loss": 4e-7, "line_loss_grad": 6e-7,
    "loss_tail": 3e-7, "loss_tail_grad": 1e-6,
    "project2d": 7e-6, "project2d_backward": 2e-5,
    "l3d": 1.5e-6, "inv_small": 3e-7, "camera": 8e-7,
    "junction_cost": 4e-7,
    "dbscan": 5e-7,
    "adam": 1e-6, "adam_moments": 2e-6,
}
UNFUSED_BAR = 1e-5          # fused against unfused loss: the bar of test_gpu_parity.test_fused_loss_tail_vs_torch_formulation


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from neat_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def both(entry, size, got, want64, want32, bar, measure=rel_err):
    """Records the kernel's and the float32 CPU formulation's error against float64 side by side; asserts the kernel's."""
    err = record("kernel", entry, size, measure(got, want64))
    record("oracle32", entry, size, measure(want32, want64))
    assert err <= bar, f"{entry} size={size}: err {err:.3e} > {bar:.1e}"


@contextmanager
def ffn_key(value):
    """Tuning key 28 (1, the default: the 256 x 256 layers and the weight gradients on the matrix pipe; 0: ffn_dense_kernel /
    ffn_backward_weights_kernel), restored afterwards."""
    from neat_amd import _lib
    lib = _lib.lib()
    _lib.check(lib.neat_set_tuning(28, value), "neat_set_tuning")
    try:
        yield lib
    finally:
        lib.neat_set_tuning(28, 1)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def poisoned(*shape, dev):
    return torch.full(shape, POISON, device=dev)


def untouched(t):
    return bool((t == POISON).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. junction MLP
# ------------------------------------------------------------------------------------------------------------------------------------
FFN_J = [1, 7, 8, 9, 31, 32, 33, 63, 65, 129, 4096, 4097]
# J <= 4096: ffn_mfma_kernel + ffn_wgrad_mfma_kernel (key 28 = 1) | ffn_dense_kernel on every layer + ffn_backward_weights_kernel (0);
# J = 4097: ffn_forward_kernel + ffn_backward_data_kernel (then the weight gradients of the key)
FFN_CASES = [(J, key) for J in FFN_J for key in (1, 0) if J <= 4096] + [(4097, 1), (4097, 0)]
FFN_PAD = 40
# seeds (found on the CPU) at which no hidden pre-activation of the float64 network lies within FFN_DELTA of zero.  FFN_DELTA is
# 50x the largest error of a hidden activation measured in test_ffn_abi_vs_float64 (3.9e-7), so kernel and reference take the same relu
# branches; without such a seed J = 129 has ~1 of its 66 048 pre-activations inside the band
FFN_DELTA = 2e-5
FFN_E2E_SEED = {1: 2100, 7: 2700, 8: 2800, 9: 2901, 31: 5100, 32: 5202, 33: 5306, 63: 8320, 65: 8518, 129: 14943}


def _ffn_ref(J, seed):
    def make():
        p, cot = jf.ffn_inputs(J, seed)
        return p, cot, jf.ffn_reference(p, cot), jf.ffn_reference(p, cot, torch.float32)
    return cached(("ffn", J, seed), make)


def _ffn_grads(entry, J, got, r64, r32):
    for k, g in zip(jf.FFN_KEYS, got):
        both(f"{entry}:d_{k}", J, g.reshape(r64["grads"][k].shape), r64["grads"][k], r32["grads"][k], BARS["ffn_backward"], rel_max)


@pytest.mark.parametrize("J,key", FFN_CASES)
def test_ffn_abi_vs_float64(dev, J, key):
    """neat_ffn_forward / neat_ffn_backward through the C ABI into oversized, poisoned buffers.  The backward kernels get the float32
    rounding of the float64 activations, so their relu masks are the reference's by construction (asserted: rounding keeps h > 0)."""
    from neat_amd import ops
    p, cot, r64, r32 = _ffn_ref(J, 1000 + J)
    for h in ("h1", "h2"):
        assert torch.equal(r64[h] > 0, r64[h].float() > 0)
    t = {k: v.to(dev) for k, v in p.items()}
    x, W0, b0, W1, b1, W2, b2 = (t[k] for k in jf.FFN_KEYS)
    h1, h2, y = poisoned(J + FFN_PAD, 256, dev=dev), poisoned(J + FFN_PAD, 256, dev=dev), poisoned(J + FFN_PAD, 3, dev=dev)
    dx, ws2 = poisoned(J + FFN_PAD, 256, dev=dev), poisoned(2 * J * 256 + FFN_PAD, dev=dev)
    dW0, db0, dW1, db1 = (poisoned(*s, dev=dev) for s in ((256, 256), (256,), (256, 256), (256,)))
    dW2, db2 = poisoned(8, 256, dev=dev), poisoned(8, dev=dev)
    from neat_amd import _lib
    with ffn_key(key) as lib:
        _lib.check(lib.neat_ffn_forward(_p(x), J, _p(W0), _p(b0), _p(W1), _p(b1), _p(W2), _p(b2), _p(h1), _p(h2), _p(y), _stream()), "ffn forward")
        lin = [types.SimpleNamespace(weight=W0, bias=b0), types.SimpleNamespace(weight=W1, bias=b1), types.SimpleNamespace(weight=W2, bias=b2)]
        with torch.no_grad():
            y_op = ops.ffn_junctions(x, lin)
        a1, a2 = r64["h1"].float().to(dev), r64["h2"].float().to(dev)
        _lib.check(lib.neat_ffn_backward(_p(x), J, _p(W0), _p(W1), _p(W2), _p(a1), _p(a2), _p(cot.to(dev)), _p(ws2), _p(dx), _p(dW0), _p(db0),
                                         _p(dW1), _p(db1), _p(dW2), _p(db2), _stream()), "ffn backward")
    tag = f"key28={key}"
    assert torch.equal(y_op, y[:J])
    both(f"ffn_forward[{tag}]:y", J, y[:J], r64["y"], r32["y"], BARS["ffn_forward"])
    both(f"ffn_forward[{tag}]:h1", J, h1[:J], r64["h1"], r32["h1"], BARS["ffn_forward"])
    both(f"ffn_forward[{tag}]:h2", J, h2[:J], r64["h2"], r32["h2"], BARS["ffn_forward"])
    for name, buf in (("h1", h1[J:]), ("h2", h2[J:]), ("y", y[J:]), ("dx", dx[J:]), ("workspace", ws2[2 * J * 256:]), ("dW2", dW2[3:]), ("db2", db2[3:])):
        assert untouched(buf), f"{tag} J={J}: {name} was written past its end"
    for name, buf in (("dW0", dW0), ("db0", db0), ("dW1", dW1), ("db1", db1), ("dW2", dW2[:3]), ("db2", db2[:3]), ("dx", dx[:J])):
        assert not bool((buf == POISON).any()), f"{tag} J={J}: {name} was not fully written"
    _ffn_grads(f"ffn_backward[{tag}]", J, (dx[:J], dW0, db0, dW1, db1, dW2[:3], db2[:3]), r64, r32)


@pytest.mark.parametrize("J,key", [(J, key) for J in FFN_J if J <= 129 for key in (1, 0)])
def test_ffn_autograd_vs_float64(dev, J, key):
    """ops.ffn_junctions end to end (the kernels' own saved activations decide the relu masks), at a seed with the margin FFN_DELTA."""
    from neat_amd import ops
    p, cot, r64, r32 = _ffn_ref(J, FFN_E2E_SEED[J])
    margin = jf.ffn_relu_margin(r64)
    assert margin > FFN_DELTA, f"J={J}: a hidden pre-activation lies {margin:.2e} from zero"
    t = [p[k].to(dev).requires_grad_(True) for k in jf.FFN_KEYS]
    lin = [types.SimpleNamespace(weight=t[1], bias=t[2]), types.SimpleNamespace(weight=t[3], bias=t[4]), types.SimpleNamespace(weight=t[5], bias=t[6])]
    with ffn_key(key):
        y = ops.ffn_junctions(t[0], lin)
        grads = torch.autograd.grad((y * cot.to(dev)).sum(), t)
    both(f"ffn_autograd[key28={key}]:y", J, y, r64["y"], r32["y"], BARS["ffn_forward"])
    _ffn_grads(f"ffn_autograd[key28={key}]", J, grads, r64, r32)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. line losses and the loss tail
# ------------------------------------------------------------------------------------------------------------------------------------
LINE_SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2049]
THR = 100.0


@pytest.mark.parametrize("L", LINE_SIZES)
def test_line_loss_vs_float64(dev, L):
    """ops.line_loss: loss, per-line error, count and d loss / d pred (x L: entries of order 1), with straight and swapped targets,
    lines beyond the gate, zero weights and rows that equal their target exactly (gradient exactly 0 on both sides)."""
    from neat_amd import ops
    pred, gt, w = jf.line_inputs(L, 300 + L)
    flip, gate, sign, zeros = jf.line_margins(pred, gt, THR)
    assert flip >= 1000.0 and gate >= 50.0 and sign >= 0.25, (flip, gate, sign)
    assert zeros == 4 * len(range(3, L, 11))
    r64, r32 = jf.line_loss_reference(pred, gt, w, THR), jf.line_loss_reference(pred, gt, w, THR, torch.float32)
    pd = pred.to(dev).requires_grad_(True)
    loss, per, count = ops.line_loss(pd, gt.to(dev), w.to(dev), THR)
    (loss * L).backward()
    assert int(count) == r64["count"]
    both("line_loss:loss", L, loss.reshape(1), r64["loss"].reshape(1), r32["loss"].reshape(1), BARS["line_loss"])
    both("line_loss:per_line", L, per, r64["per_line"], r32["per_line"], BARS["line_loss"])
    both("line_loss:d_pred", L, pd.grad, r64["d_pred"] * L, r32["d_pred"] * L, BARS["line_loss_grad"], rel_max)
    assert torch.equal(pd.grad.cpu() == 0, r64["d_pred"] == 0)


def _pair_case(i):
    return [(0, 64, "all"), (1, 1, "all"), (5, 64, "all"), (70, 64, "all"), (64, 1024, "some"), (5, 64, "none")][i % 6]


# (L = R, E, (K, J, good)): every size of each list at least once; both with and without the lines3d / w2c fold
TAIL_CASES = [(n, [0, 1, 1025][i % 3]) + _pair_case(i) for i, n in enumerate(LINE_SIZES)] + [(65, 1025, 5, 64, "none"), (1025, 0, 64, 1024, "some")]
SCALARS = ("rgb_loss", "eikonal_loss", "j3d_loss", "j2d_loss", "j2d_stat", "loss", "l2d_loss", "line_loss")


def _tail_margins(inp, fold):
    """Every branch of the loss tail, from float64 alone."""
    L = inp["pred_px"].shape[0]
    flip, gate, _, _ = jf.line_margins(inp["pred_px"], inp["gt5"][:, :4], THR)
    assert flip >= 1000.0 and gate >= 50.0, (flip, gate)
    w2c = jf.f64(inp["w2c"])
    pc = jf.O.project2d(torch.eye(3, dtype=F64), w2c[:, :3], w2c[:, 3:], jf.f64(inp["lines3d"])).reshape(L, 4) if fold else inp["pred_calib"]
    flip, gate, sign, zeros = jf.line_margins(pc, jf.calibrate64(inp["K"], inp["gt5"][:, :4]), THR)
    assert flip >= 1e-3 and gate >= 50.0 and sign >= 5e-4 and zeros == 0, (flip, gate, sign, zeros)
    d = jf.f64(inp["rgb"]) - jf.f64(inp["rgb_gt"])
    assert bool(((d == 0) | (d.abs() >= 5e-3)).all()) and int((d == 0).sum()) == 3 * len(range(1, d.shape[0], 6))
    if "gtheta" in inp:
        nrm = jf.f64(inp["gtheta"]).norm(dim=1)
        assert bool(((nrm == 0) | (nrm >= 0.4)).all())


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("n,E,K,J,good_mode", TAIL_CASES)
def test_loss_tail_vs_float64(dev, n, E, K, J, good_mode, fold):
    """ops.loss_tail (line_losses_body + loss_terms_body in one launch, neat_lsap, loss_pairs_kernel) against oracle.neat_loss in
    float64: every scalar of `scal` and `line3`, every gradient it returns, and the matching (scipy on the float64 pair cost, unique by
    the asserted gap).

    With no matched pair (K = 0, or `good` all false) the kernels return 0 for j3d / j2d / j2d_stat / jcount.  So does the oracle,
    which compacts the local junctions with `[good]` first and skips the junction terms when none is left (neat_loss: `if
    res["j3d_local"].shape[0] > 0`), and so does the unfused path of neat_amd/loss.py, which divides the masked sums by
    max(n_match, 1): asserted against both."""
    from neat_amd import ops
    from neat_amd.loss import VolSDFLoss
    inp = cached(("tail", n, E, K, J, good_mode), lambda: jf.tail_inputs(n, n, E, K, J, good_mode, 7000 + n + K))
    _tail_margins(inp, fold)
    w_eik, w_line, w_j3, w_j2 = 0.1, 0.01, 0.1, 0.01
    s64, g64 = jf.tail_reference(inp, fold)
    s32, g32 = jf.tail_reference(inp, fold, torch.float32)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
    leaves = {k: d[k].clone().requires_grad_(True) for k in g64}
    have = K > 0
    if have and good_mode != "none":
        cost = jf.pair_cost64(inp)
        ri, ci, gap, worst = jf.matching_margin(cost, inp["good"])
        far = cost[ri, ci] >= 10
        assert gap >= 0.02 and bool(((cost[ri, ci] < 5) | (cost[ri, ci] > 11)).all()), (gap, worst)
        assert int(far.sum()) == (1 if 5 <= K <= J else 0)
        rows, cols, n_match = ops.linear_sum_assignment(cost.float().to(dev), d["good"])
        m = int(n_match)
        assert m == len(ri) and torch.equal(rows[:m].cpu(), ri) and torch.equal(cols[:m].cpu(), ci)
    eye34 = torch.eye(3, 4, device=dev)
    with torch.no_grad():
        if fold:
            pc = ops.project2d(eye34[:, :3].contiguous(), d["w2c"], leaves["lines3d"]).reshape(-1, 4)
            glo2c = ops.project2d(eye34[:, :3].contiguous(), d["w2c"], leaves["glo3"]) if have else None
    if not fold:
        pc, glo2c = leaves["pred_calib"], leaves.get("glo2c") if have else None
    loss, scal, line3 = ops.loss_tail(leaves["rgb"], leaves.get("gtheta"), leaves["glo3"] if have else None, glo2c, pc, d["pred_px"], d["gt5"], d["K"],
                                      d["rgb_gt"], d["loc3"] if have else None, d["loc2c"] if have else None, d["loc2"] if have else None,
                                      d["glo2"] if have else None, d["good"] if have else None, w_eik, w_line, w_j3, w_j2, THR,
                                      leaves["lines3d"] if fold else None, d["w2c"] if fold else None)
    names = [k for k in g64 if have or k not in ("glo3", "glo2c")]
    grads = dict(zip(names, torch.autograd.grad(loss, [leaves[k] for k in names])))
    got = dict(rgb_loss=scal[0], eikonal_loss=scal[1], j3d_loss=scal[2], j2d_loss=scal[3], j2d_stat=scal[4], loss=loss, l2d_loss=line3[0],
               line_loss=line3[1])
    tag = f"loss_tail[fold={int(fold)}]"
    size = f"L{n}-E{E}-K{K}-J{J}-{good_mode}"
    assert int(line3[2]) == int(s64["count"]) and int(scal[5]) == int(s64["jcount"]), (line3[2], s64["count"], scal[5], s64["jcount"])
    if have:
        assert float(scal[6]) == float(loss)
    for k in SCALARS:
        both(f"{tag}:{k}", size, got[k].reshape(1), s64[k].reshape(1), s32[k].reshape(1), BARS["loss_tail"])
    for k in names:
        both(f"{tag}:d_{k}", size, grads[k], g64[k], g32[k], BARS["loss_tail_grad"], rel_max)
        assert torch.equal(grads[k].cpu() == 0, g64[k] == 0), k
    if not have or good_mode == "none":
        for k in ("j3d_loss", "j2d_loss", "j2d_stat"):
            assert float(got[k]) == 0.0 and float(s64[k]) == 0.0
        assert float(scal[5]) == 0.0
        if not fold:        # the unfused path of neat_amd/loss.py on the same tensors
            out = _Outputs({"rgb_values": d["rgb"], "lines2d": d["pred_px"], "lines2d_calib": d["pred_calib"], "K": d["K"]})
            if "gtheta" in d:
                out["grad_theta"] = d["gtheta"]
            out.good = d["good"] if have else None
            out.padded = {"j3d_local": d["loc3"] if have else torch.zeros(0, 3, device=dev), "j2d_local_calib": d.get("loc2c"), "j2d_local": d.get("loc2")}
            if have:
                out.update(j3d_global=d["glo3"], j2d_global_calib=d["glo2c"], j2d_global=d["glo2"])
            lf = VolSDFLoss("torch.nn.L1Loss", w_eik, w_line, w_j3, w_j2)
            lf.fused_tail = False
            lo = lf(out, {"rgb": d["rgb_gt"], "lines2d": d["gt5"][None]})
            for k in ("j3d_loss", "j2d_loss", "j2d_stat", "jcount"):
                assert float(lo[k]) == 0.0, k
            assert abs(float(lo["loss"].detach()) - float(loss.detach())) <= UNFUSED_BAR * max(1.0, abs(float(loss.detach())))


class _Outputs(dict):
    """Model outputs as neat_amd.loss reads them: a dict with the padded matched junctions and their mask as attributes."""


@pytest.mark.parametrize("L", LINE_SIZES)
def test_line_losses_vs_float64(dev, L):
    """ops.line_losses (line_losses_kernel: both line terms and the K^-1 calibration between them) against oracle.neat_loss."""
    from neat_amd import ops
    inp = cached(("tail", L, 0, 0, 0, "all"), lambda: jf.tail_inputs(L, L, 0, 0, 0, "all", 7000 + L))
    _tail_margins(inp, False)
    s64, g64 = jf.tail_reference(inp, False, weights=(0.0, float(L), 0.0, 0.0))
    s32, g32 = jf.tail_reference(inp, False, torch.float32, weights=(0.0, float(L), 0.0, 0.0))
    pc = inp["pred_calib"].to(dev).requires_grad_(True)
    l2d, ll, count = ops.line_losses(inp["pred_px"].to(dev), pc, inp["gt5"].to(dev), inp["K"].to(dev), THR)
    (ll * L).backward()
    assert int(count) == int(s64["count"])
    both("line_losses:l2d_loss", L, l2d.reshape(1), s64["l2d_loss"].reshape(1), s32["l2d_loss"].reshape(1), BARS["line_loss"])
    both("line_losses:line_loss", L, ll.reshape(1), s64["line_loss"].reshape(1), s32["line_loss"].reshape(1), BARS["line_loss"])
    both("line_losses:d_pred_calib", L, pc.grad, g64["pred_calib"], g32["pred_calib"], BARS["line_loss_grad"], rel_max)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. projections, l3d, camera glue, the small inverse
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_project2d_vs_float64(dev, N):
    """project2d, project2d_pair and their backward at |cam_z| >= 0.1 (asserted), both signs, a K with skew."""
    from neat_amd import ops
    K, w2c, X, cot, cot2 = jf.proj_inputs(N, 400 + N)
    eye = torch.eye(3)
    ref = {(n, dt): jf.project_reference(Km, w2c, X, c, dt) for n, Km, c in (("K", K, cot), ("I", eye, cot2)) for dt in (F64, torch.float32)}
    for n in ("K", "I"):
        assert float(ref[(n, F64)][2].abs().min()) >= 0.09
    Xd = X.to(dev).requires_grad_(True)
    uv = ops.project2d(K.to(dev), w2c.to(dev), Xd)
    (gX,) = torch.autograd.grad((uv * cot.to(dev)).sum(), Xd)
    both("project2d", N, uv, ref[("K", F64)][0], ref[("K", torch.float32)][0], BARS["project2d"])
    both("project2d:backward", N, gX, ref[("K", F64)][1], ref[("K", torch.float32)][1], BARS["project2d_backward"], rel_max)
    a, b = ops.project2d_pair(K.to(dev), eye.to(dev), w2c.to(dev), Xd)
    assert torch.equal(a, uv)
    both("project2d_pair:calibrated", N, b, ref[("I", F64)][0], ref[("I", torch.float32)][0], BARS["project2d"])
    (gX2,) = torch.autograd.grad((a * cot.to(dev)).sum() + (b * cot2.to(dev)).sum(), Xd)
    both("project2d_pair:backward", N, gX2, ref[("K", F64)][1] + ref[("I", F64)][1], ref[("K", torch.float32)][1] + ref[("I", torch.float32)][1],
         BARS["project2d_backward"], rel_max)


def test_project2d_guarded_depth(dev):
    """cam_z exactly +0, -0 and +-5e-9 (inside the |w| < 1e-8 guard: w +- 1e-8), +-2e-8 (outside it).  With K's last row (0, 0, 1) and
    [I | 0] the kernel's cam_z IS the point's z, bit for bit, so kernel and reference take the same branch."""
    from neat_amd import ops
    K = torch.tensor(jf.K_SKEW)
    w2c = torch.eye(3, 4)
    z = torch.tensor([0.0, -0.0, 5e-9, -5e-9, 2e-8, -2e-8])
    X = torch.cat([torch.tensor([[0.3, -0.2], [0.1, 0.4], [-0.5, 0.2], [0.2, 0.2], [0.7, -0.1], [-0.3, -0.6]]), z[:, None]], 1)
    ref64, _, depth = jf.project_reference(K, w2c, X, torch.zeros(6, 2))
    ref32, _, _ = jf.project_reference(K, w2c, X, torch.zeros(6, 2), torch.float32)
    assert torch.equal(depth, z.double()) and bool(((depth.abs() < 1e-8) == torch.tensor([1, 1, 1, 1, 0, 0], dtype=torch.bool)).all())
    uv = ops.project2d(K.to(dev), w2c.to(dev), X.to(dev))
    both("project2d:guarded", 6, uv, ref64, ref32, BARS["project2d"])
    a, b = ops.project2d_pair(K.to(dev), K.to(dev), w2c.to(dev), X.to(dev))
    assert torch.equal(a, uv) and torch.equal(b, uv)
    assert torch.equal(torch.sign(uv.cpu()).double(), torch.sign(ref64))


@pytest.mark.parametrize("R", [1, 255, 257])
def test_l3d_vs_float64(dev, R):
    from neat_amd import ops
    x, o, d, n = jf.l3d_inputs(R, 500 + R)
    ref64, den = jf.l3d_reference(x, o, d, n)
    assert float(den.abs().min()) >= 0.05
    got = ops.l3d_points(x.to(dev), o.to(dev), d.to(dev), n.to(dev))
    both("l3d", R, got, ref64, jf.l3d_reference(x, o, d, n, torch.float32)[0], BARS["l3d"])


def test_l3d_ray_in_the_plane(dev):
    """<d, n> exactly 0 (axis vectors): the denominator is the +1e-6 of the guard on both sides."""
    from neat_amd import ops
    d = torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    n = torch.tensor([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    x, o = torch.tensor([[0.5, 0.25, 1.0], [0.125, 2.0, 0.5], [1.0, 1.0, 0.375]]), torch.tensor([[0.0, 0.5, 0.0], [0.25, 0.0, 1.0], [0.5, 0.5, 0.5]])
    ref64, den = jf.l3d_reference(x, o, d, n)
    assert bool((den == 0).all())
    got = ops.l3d_points(x.to(dev), o.to(dev), d.to(dev), n.to(dev))
    both("l3d:in_plane", 3, got, ref64, jf.l3d_reference(x, o, d, n, torch.float32)[0], BARS["l3d"])


# row exchanges that a float64 elimination with partial pivoting makes (a cyclic permutation of three rows is undone by two)
INV_EXCHANGES = {"n2_swap": 1, "n3_K_rows_exchanged": 1, "n3_cycle": 2, "n4_pose_cycle": 2, "n4_pose_cycle_tilted": 2, "n4_shift": 3}


@pytest.mark.parametrize("name", sorted(jf.inv_matrices()))
def test_inv_small_vs_float64(dev, name):
    """inv_small_kernel, n = 1 .. 4, with lda = n (ops.inv_small) and lda = n + 3 through the ABI; the matrices of INV_EXCHANGES have
    a zero (or tiny) leading entry at every elimination step that still has a row to exchange with (asserted on a float64
    elimination)."""
    from neat_amd import _lib, ops
    A = jf.inv_matrices()[name]
    n = A.shape[0]
    assert jf.swaps_needed(A) >= INV_EXCHANGES.get(name, 0), jf.swaps_needed(A)
    ref64, ref32 = torch.linalg.inv(A.double()), torch.linalg.inv(A)
    got = ops.inv_small(A.to(dev))
    both(f"inv_small:{name}", n, got, ref64, ref32, BARS["inv_small"])
    wide = poisoned(n, n + 3, dev=dev)
    wide[:, :n] = A.to(dev)
    out = poisoned(n * n + 4, dev=dev)
    _lib.check(_lib.lib().neat_inv_small(_p(wide), n, n + 3, _p(out), _stream()), "neat_inv_small")
    assert torch.equal(out[:n * n].view(n, n), got) and untouched(out[n * n:])


@pytest.mark.parametrize("with_proj", [False, True])
@pytest.mark.parametrize("kdim", [3, 4])
@pytest.mark.parametrize("R", [1, 255, 257])
def test_camera_setup_vs_float64(dev, R, kdim, with_proj):
    """camera_setup (and camera_mats on the same camera): dirs, origins, w2c and K3 against oracle.camera_rays and the float64
    inverse, intrinsics with row stride 3 and 4, a random pose and one whose rotation needs a row exchange at every step."""
    from neat_amd import ops
    g = jf.gen(600 + R)
    uv, uv2 = torch.rand(1, R, 2, generator=g) * 512, torch.rand(1, R, 2, generator=g) * 512
    Kin = torch.eye(kdim)
    Kin[:3, :3] = torch.tensor(jf.K_SKEW)
    for pname, pose in (("random", jf.random_pose(R)), ("cycle", jf.pivot_pose(R, 0.01))):
        r64, r32 = jf.camera_reference(uv, pose, Kin), jf.camera_reference(uv, pose, Kin, torch.float32)
        dirs, origins, dirs2, w2c, K3 = ops.camera_setup(uv.to(dev), uv2.to(dev) if with_proj else None, pose[None].to(dev), Kin[None].to(dev))
        tag = f"camera_setup[{pname},k{kdim}]"
        both(f"{tag}:dirs", R, dirs, r64[0], r32[0], BARS["camera"])
        both(f"{tag}:origins", R, origins, r64[1].expand(R, 3), r32[1].expand(R, 3), BARS["camera"])
        both(f"{tag}:w2c", R, w2c, r64[2], r32[2], BARS["camera"])
        assert torch.equal(K3.cpu(), Kin[:3, :3])
        if with_proj:
            q64, q32 = jf.camera_reference(uv2, pose, Kin), jf.camera_reference(uv2, pose, Kin, torch.float32)
            both(f"{tag}:dirs_proj", R, dirs2, q64[0], q32[0], BARS["camera"])
        else:
            assert dirs2 is None
        w2c_m, K3_m = ops.camera_mats(pose.to(dev), Kin.to(dev))
        assert torch.equal(w2c_m, w2c) and torch.equal(K3_m, K3)


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. junction cost and gate
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,C", [(1, 1), (23, 500), (2048, 3)])
def test_junction_cost_vs_float64(dev, V, C):
    from neat_amd import ops
    g = jf.gen(V + C)
    cand, gt = torch.rand(C, 2, generator=g) * 512, torch.rand(V, 2, generator=g) * 512
    cost = ops.junction_cost(cand.to(dev), gt.to(dev))
    both("junction_cost", f"{V}x{C}", cost, jf.junction_cost_reference(cand, gt), jf.junction_cost_reference(cand, gt, torch.float32),
         BARS["junction_cost"])


@pytest.mark.parametrize("K", [1, 2, 1023, 1025, 2048])
def test_junction_gate_exact(dev, K):
    """junction_gate_kernel, both gates: K and K - 1 valid pairs (an even and an odd count), costs quantised to quarters (the median
    value occurs several times), every pair -1, costs of exactly 10.0 at the fixed gate.  The reference compares and gathers the same
    float32 numbers, so every output is equal bit for bit."""
    from neat_amd import ops
    g = jf.gen(800 + K)
    C = K + 3
    cost = torch.rand(K, C, generator=g) * 20
    cand3d, cand2d, cand2dc = torch.randn(C, 3, generator=g), torch.rand(C, 2, generator=g) * 512, torch.randn(C, 2, generator=g)
    rows, cols = torch.arange(K), torch.randperm(C, generator=g)[:K]
    quant = (cost * 4).round() / 4
    ten = cost.clone()
    ten[rows[::3], cols[::3]] = 10.0
    cases = {"all": (rows, cols, cost), "one_dropped": (rows.clone(), cols.clone(), cost), "duplicates": (rows, cols, quant),
             "duplicates_dropped": (rows.clone(), cols.clone(), quant), "none": (torch.full((K,), -1), torch.full((K,), -1), cost), "ten": (rows, cols, ten)}
    for name in ("one_dropped", "duplicates_dropped"):
        cases[name][0][K // 2], cases[name][1][K // 2] = -1, -1
    for name, (r, c, cst) in cases.items():
        if name.startswith("duplicates") and K >= 1023:
            m = cst[rows, cols]
            assert int((m == torch.median(m)).sum()) >= 3
        for use_median in (True, False):
            med, good, j3, j2, j2c = jf.gate_reference(r, c, cst, cand3d, cand2d, cand2dc, use_median)
            got = ops.junction_gate(r.to(dev), c.to(dev), cst.to(dev), cand3d.to(dev), cand2d.to(dev), cand2dc.to(dev), use_median)
            what = (name, use_median)
            if use_median:
                assert float(got[0]) == float(med), what
            else:
                assert got[0] is None
            assert torch.equal(got[1].cpu(), good), what
            assert torch.equal(got[2].cpu(), j3) and torch.equal(got[3].cpu(), j2) and torch.equal(got[4].cpu(), j2c), what
        if name == "ten":
            assert not bool(jf.gate_reference(r, c, cst, cand3d, cand2d, cand2dc, False)[1][::3].any())


def test_junction_gate_refuses_more_than_2048_pairs(dev):
    """The gate keeps the matched costs in LDS (2048 floats): K = 2049 is refused by the host and nothing is launched (the outputs keep
    their poison).  neat_amd.networks only takes this path for min(V, C) <= 2048."""
    from neat_amd import _lib, ops
    K = 2049
    rows = cols = torch.arange(K, device=dev)
    cost, c3, c2 = torch.ones(K, K, device=dev), torch.zeros(K, 3, device=dev), torch.zeros(K, 2, device=dev)
    with pytest.raises(RuntimeError):
        ops.junction_gate(rows, cols, cost, c3, c2, c2, True)
    med, good = poisoned(1, dev=dev), torch.full((K,), 7, dtype=torch.uint8, device=dev)
    j3, j2, j2c = poisoned(K, 3, dev=dev), poisoned(K, 2, dev=dev), poisoned(K, 2, dev=dev)
    rc = _lib.lib().neat_junction_gate(_p(rows), _p(cols), K, _p(cost), K, _p(c3), _p(c2), _p(c2), 1, _p(med), _p(good), _p(j3), _p(j2), _p(j2c), _stream())
    torch.cuda.synchronize()
    assert rc != 0 and untouched(med) and untouched(j3) and untouched(j2) and untouched(j2c) and bool((good == 7).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. DBSCAN means
# ------------------------------------------------------------------------------------------------------------------------------------
def _dbscan_check(dev, pts, entry):
    from neat_amd import ops
    n = pts.shape[0]
    ref, near = jf.dbscan_reference(pts)
    assert near == 0, f"{near} point pairs lie on the eps boundary"
    got, valid, count = ops.dbscan_means(torch.tensor(pts).to(dev), 0.01)
    k = int(count)
    assert got.shape == (n // 2, 3) and k == ref.shape[0] and int(valid.sum()) == k and bool(valid[:k].all())
    err = record("kernel", entry, n, rel_err(got[:k], ref))
    labels = _labels(pts)
    record("oracle32", entry, n, rel_err(torch.tensor(np.array([pts[labels == i].mean(axis=0) for i in range(k)]).reshape(-1, 3)), ref))
    assert err <= BARS["dbscan"], (entry, n, err)
    assert float(got[k:].abs().sum()) == 0.0
    return k


def _labels(pts):
    from sklearn.cluster import DBSCAN
    return DBSCAN(eps=0.01, min_samples=2).fit(pts).labels_


# mode 2 of dbscan_finish_kernel (fixed-point LDS sums) up to n = 5461, mode 1 (one wavefront per cluster) from 5462; odd n: n/2 slots
@pytest.mark.parametrize("n", [2, 3, 65, 4097, 5461, 5462, 8191])
def test_dbscan_means_vs_float64(dev, n):
    """The blobs / noise / chain construction of test_lsap.py against sklearn's clusters and float64 means (seeds at which no pair of
    points lies on the eps boundary: asserted)."""
    _dbscan_check(dev, jf.dbscan_points(n, {8191: 8192}.get(n, n)), "dbscan_means")


@pytest.mark.parametrize("n", [2, 3, 65, 5461, 5462])
def test_dbscan_all_noise_and_one_chain(dev, n):
    """No two points within eps: count 0, nothing valid, centres all zero.  One chain of 0.004 steps: a single cluster of all n points."""
    i = np.arange(n)
    noise = np.stack([(i % 32) * 0.05, (i // 32 % 32) * 0.05, (i // 1024) * 0.05], 1).astype(np.float32) - 0.8
    assert _dbscan_check(dev, noise, "dbscan_means:noise") == 0
    chain = (np.array([-0.9, 0.3, 0.1]) + i[:, None] * np.array([0.004 * 0.6, 0.004 * 0.8, 0.0]) * (0.3 if n > 4096 else 1.0)).astype(np.float32)
    assert _dbscan_check(dev, chain, "dbscan_means:chain") == 1


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. Adam
# ------------------------------------------------------------------------------------------------------------------------------------
ADAM_LAYOUTS = {"edges": [1, 2, 3, 4, 5, 7, 1019, 1, 1024, 1025, 4093], "96_small": [1 + (7 * k) % 9 for k in range(96)], "one": [4]}
ADAM_KEEP = (1, 2, 10)
LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("layout", sorted(ADAM_LAYOUTS))
def test_flat_adam_vs_float64(dev, layout, flat):
    """FlatAdam after steps 1, 2 and 10: parameters, both moments (per tensor, relative to the tensor's own scale) and the step counts
    of state_dict().  `.grad` form: the first, a middle and the last tensor take turns without a gradient (no step, as torch.optim.Adam);
    `flat_grad=` form: every tensor steps, a missing gradient is zeros (the moments decay), and tensors at odd offsets hand the kernel
    gradient pointers that are not 16-byte aligned (its scalar-load path); `edges` has n % 4 != 0 and segment boundaries at elements
    1023 / 1024 / 1025 of a 1024-element block (the straddling loop).

    The hyper-parameters of the reference are the float32 roundings the C ABI receives (beta2 = 0.99900001287): against the double
    0.999 the kernel's exp_avg_sq is 4.7e-5 off in relative terms, since 1 - float32(0.999) = 1.0000467e-3 -- as large for the float32
    CPU formulation with the same rounded betas, and without effect on the parameters (the bias correction uses the same beta2)."""
    from neat_amd.optim import FlatAdam
    sizes = ADAM_LAYOUTS[layout]
    nt = len(sizes)
    p0, grads = jf.adam_inputs(sizes, max(ADAM_KEEP), 900 + nt)
    skip = [0, nt // 2, nt - 1]
    for t, row in enumerate(grads):
        k = skip[t % 3]
        if nt > 1 or t % 3 == 1:                 # (the single tensor of `one` goes without a gradient at every third step only)
            row[k] = torch.zeros_like(row[k]) if flat else None
    hyper = (jf.f32(LR), (jf.f32(BETAS[0]), jf.f32(BETAS[1])), jf.f32(EPS))
    r64 = jf.adam_reference(p0, grads, *hyper, ADAM_KEEP)
    r32 = jf.adam_reference(p0, grads, *hyper, ADAM_KEEP, torch.float32)
    params = [torch.nn.Parameter(t.clone().to(dev)) for t in p0]
    opt = FlatAdam(params, lr=LR, betas=BETAS, eps=EPS)
    flat_grad = torch.zeros(sum(sizes), device=dev) if flat else None
    tag = f"adam[{layout},{'flat_grad' if flat else 'grad'}]"
    for t, row in enumerate(grads, 1):
        if flat:
            flat_grad.copy_(torch.cat(row).to(dev))
            opt.step(flat_grad=flat_grad)
        else:
            for prm, gk in zip(params, row):
                prm.grad = None if gk is None else gk.to(dev)
            opt.step()
        if t not in ADAM_KEEP:
            continue
        st = opt.state_dict()["state"]
        assert [int(st[i]["step"]) for i in range(nt)] == r64[t][3], (t, [int(st[i]["step"]) for i in range(nt)], r64[t][3])
        for i in range(nt):
            size = f"step{t}"
            both(f"{tag}:param", size, params[i], r64[t][0][i], r32[t][0][i], BARS["adam"])
            both(f"{tag}:exp_avg", size, st[i]["exp_avg"], r64[t][1][i], r32[t][1][i], BARS["adam_moments"], rel_max)
            both(f"{tag}:exp_avg_sq", size, st[i]["exp_avg_sq"], r64[t][2][i], r32[t][2][i], BARS["adam_moments"], rel_max)
    if flat and nt > 1:
        assert any((4 * sum(sizes[:i])) % 16 for i in range(nt))      # some gradient pointers are misaligned


def test_flat_adam_refuses_97_tensors(dev):
    from neat_amd.optim import FlatAdam
    with pytest.raises(ValueError):
        FlatAdam([torch.nn.Parameter(torch.zeros(2, device=dev)) for _ in range(97)], lr=LR)
