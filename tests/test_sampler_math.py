"""CPU-only checks of tests/sampler_f64.py, the references and bars of tests/test_f64_sampler_edges.py: every condition on left-out
rays and samples holds at every size the GPU tests name, the constants recorded there are what this machine measures, the emulation of
the kernel's arithmetic stays within the bars, and the plain-torch references equal torch.sort / torch.searchsorted compositions."""
import pytest
import torch

from oracle import neat_oracle as O
from tests import sampler_f64 as S
from tests.sampler_f64 import F32, F64, f64

ALL_N = S.SIZES + (960,)
RESAMPLE_U = [(1, "shared"), (2, "shared"), (64, "shared"), (65, "shared"), (257, "shared"), (64, "per_ray")]


def u_of(R, N, kind):
    return S.u_shared(N) if kind == "shared" else S.u_per_ray(R, N)


@pytest.mark.parametrize("n", ALL_N)
def test_bisection_conditions_and_tau(n):
    """<= 25 % of the rays inside the margin, an open and a closed ray kept; TAU is at least 8 x the float32-float64 difference."""
    cases = [S.bound_case(n)] + [S.bound_case(n, N) for N in (1, 64) if n - N >= 1]
    cases += [S.bound_case(n, iters=it) for it in (0, 1)]
    for c in cases:
        S.assert_bound_conditions(c)
        assert bool((c["beta"] >= S.BETA0).all()) and bool((c["beta"] <= c["beta_in"].clamp_min(S.BETA0)).all())
    for c in cases[:3]:
        diff = S.bound_f32_vs_f64(c["z"], c["sdf"], c["beta_in"])
        assert 8 * diff <= S.TAU, diff


@pytest.mark.parametrize("refine", [True, False])
@pytest.mark.parametrize("n", ALL_N)
def test_cdf_conditions_and_emulation(n, refine):
    """Half of the rays and half of the open rays are compared; the emulation of the kernel's arithmetic stays below K_EMUL_MEASURED x
    bound in every knot and within the bar in every compared sample; at most 10 % of the case's samples are left out."""
    c = S.cdf_case(n, refine)
    S.assert_cdf_conditions(c)
    assert S.emulation_ratio(c, refine) <= S.K_EMUL_MEASURED
    k = c["kept"] & ~c["zero_pdf"]
    z32, z64 = c["z"][k], f64(c["z"])[k]
    emu = S.cdf_emulation(c["z"], c["sdf"], c["beta"], refine)[k]
    out = total = 0
    for N, kind in RESAMPLE_U:
        u = u_of(c["z"].shape[0], N, kind)
        uk = u if u.dim() == 1 else u[k]
        ref, bar, cmp_ = S.sample_bars(z64, c["cdf"][k], uk, c["bar"][k])
        got = f64(O._inverse_cdf(z32, emu, uk.expand(z32.shape[0], -1).contiguous()))
        assert bool(((got - ref).abs() <= bar)[cmp_].all()), float(((got - ref).abs() / bar)[cmp_].max())
        out, total = out + int((~cmp_).sum()), total + cmp_.numel()
    assert out <= 0.1 * total, (out, total)


def test_add_tiny_makes_a_zero_pdf_ray_finite():
    c0, c1 = S.cdf_case(2, True), S.cdf_case(2, True, add_tiny=1e-6)
    assert bool(c0["zero_pdf"].any()) and not bool(c1["zero_pdf"].any())
    assert bool((c1["kept"] & c0["zero_pdf"]).any())


def test_bisection_equals_the_oracle_sampler_in_float64():
    """oracle.error_bound_sampler's first-round betas (float64 run, n = 128) against S.bisect on the same float32 grid and sdf values.
    The oracle's midpoints are float64, S.bisect's float32: a ray with a margin agrees to a rounding, a flipped decision would move
    beta by 2^-10 of the interval."""
    R, n = 48, 128
    g = S.gen(11)
    h = f64(torch.rand(R, generator=g) * 1.5)
    origin = torch.tensor([0.0, 0.0, -3.0], dtype=F64)
    ends = torch.stack([h, torch.zeros_like(h), torch.zeros_like(h)], -1)
    dirs = torch.nn.functional.normalize(ends - origin, dim=-1)
    sdf_fn = lambda p: (p.norm(dim=-1) - 1.0).to(F32).to(F64)
    beta0 = f64(torch.tensor(S.BETA0, dtype=F32))
    trace = {}
    O.error_bound_sampler(sdf_fn, beta0, dirs, origin[None], training=False, rand={"eik_idx": torch.zeros(R, dtype=torch.long)},
                          n_eval=n, eps=S.EPS, beta_iters=S.ITERS, max_iters=1, trace=trace)
    z = O.uniform_z(R, n, 0.0, 6.0)
    sdf = sdf_fn(origin[None, None] + z.to(F64)[:, :, None] * dirs[:, None, :]).to(F32)
    beta, margin = S.bisect(z, sdf, S.beta_init(z), beta0=float(beta0))
    kept = margin >= S.TAU
    assert int(kept.sum()) >= R // 2 and bool((beta[kept] > S.BETA0).any()) and bool((beta[kept] == beta0.to(F32)).any())
    want = trace["beta"][0]
    assert bool(((f64(beta) - want).abs() <= 1e-6 * want)[kept].all())


@pytest.mark.parametrize("nb,N,zeros", S.PDF_CASES)
def test_sample_pdf_reference(nb, N, zeros):
    """The float64 sample_pdf reference is a searchsorted composition; the empty bins keep a third from the rule; <= 10 % left out."""
    bins, w = S.pdf_inputs(nb, zeros=zeros)
    R = bins.shape[0]
    for u in (S.u_shared(N), S.u_per_ray(R, N)):
        ref, bar, cmp_, den = S.pdf_reference(bins, w, u)
        b64, u64 = f64(bins), f64(u).expand(R, -1).contiguous()
        cdf = torch.cat([torch.zeros(R, 1, dtype=F64), torch.cumsum((f64(w) + 1e-5) / (f64(w) + 1e-5).sum(-1, keepdim=True), -1)], -1)
        idx = torch.searchsorted(cdf, u64, right=True)
        lo, hi = (idx - 1).clamp(min=0), idx.clamp(max=nb - 1)
        d = cdf.gather(1, hi) - cdf.gather(1, lo)
        want = b64.gather(1, lo) + (u64 - cdf.gather(1, lo)) / torch.where(d < 1e-5, torch.ones_like(d), d) * (b64.gather(1, hi) - b64.gather(1, lo))
        assert torch.equal(ref, want)
        if zeros:
            assert bool((f64(w).sum(-1) >= 1.5).all()) and bool((w == 0).any()) and S.rule_margin(den) >= 1.0 / 3.0
        assert float((~cmp_).float().mean()) <= 0.1


def test_merge_and_finish_references_equal_torch_sort():
    g = S.gen(3)
    for n, N in ((2, 1), (65, 64), (257, 257), (1024, 64)):
        z = (torch.rand(5, n, generator=g) * 6).sort(-1)[0]
        s = (torch.rand(5, N, generator=g) * 6).sort(-1)[0]
        s[:, 0] = z[:, 0]                                    # ties: old first
        s[:, -1] = z[:, -1]
        s = s.sort(-1)[0]
        merged, order = S.merge_reference(z, s)
        want, worder = torch.sort(torch.cat([z, s], -1), dim=-1, stable=True)
        assert torch.equal(merged, want) and torch.equal(order, worder)
    for M in (2, 3, 64, 65, 1024):
        rows = torch.rand(4, M, generator=g)
        rows[:, M // 2] = rows[:, 0]
        assert torch.equal(S.rank_sort(rows), torch.sort(rows, -1)[0])
    keys = S.keys_with_ties(771)
    for n in (37, 257, 771):
        p = S.picks_reference(keys, n, 32)
        assert torch.equal(keys[p], torch.sort(keys[:n])[0][:32]) and p.unique().numel() == 32


def test_tied_keys_rank_among_the_picks_of_every_grid():
    """The picks the GPU tests compare hold equal keys in every grid, and in every grid of more than one 256-key part a pair whose
    indices lie in different parts: the lower-index-first rule across parts decides the order that is compared."""
    for n_step, n_cand in ((37, 5), (128, 8), (257, 3)):
        keys = S.keys_with_ties(n_step * n_cand)
        for c in range(n_cand):
            n = n_step * (c + 1)
            p = S.picks_reference(keys, n, 32)
            assert keys[p].unique().numel() < 32, (n_step, n)
            assert n <= 256 or S.tied_pair_across_parts(keys, p), (n_step, n)
    for n in (37, 257, 1023):                                   # the one-workgroup pick of neat_sampler_finish_dev
        keys = S.keys_with_ties(n, seed=1)
        p = S.picks_reference(keys, n, 32)
        assert keys[p].unique().numel() < 32 and (n <= 256 or S.tied_pair_across_parts(keys, p)), n


@pytest.mark.parametrize("nb,N,zeros", S.PDF_CASES)
def test_sample_pdf_bars_hold_the_emulation_and_catch_a_dropped_carry(nb, N, zeros):
    bins, w = S.pdf_inputs(nb, zeros=zeros)
    u = S.u_per_ray(bins.shape[0], 64)
    ref, bar, cmp_, _ = S.pdf_reference(bins, w, u)
    within = lambda got: bool(((f64(got) - ref).abs() <= bar)[cmp_].all())
    assert within(S.pdf_emulation(bins, w, u))
    if nb - 1 > 64:
        assert not within(S.pdf_emulation(bins, w, u, carry=False))


def test_cdf_bars_catch_a_wrong_wave_offset():
    """A knot prefix that misses one wave's total (the defect the PER = 5 sizes are there to catch) leaves the sample bars at once --
    where the ray's mass is: with z uniform in [0, 6] the sphere's near surface lies in the second wave's knots (320 .. 639 of 1024),
    so the offsets of waves 1 and 2 decide where the samples go.  The last wave's knots lie behind the surface, in empty bins at the
    `den < 1e-5` rule, and the same defect there moves no compared sample of the final pdf (asserted too, so that nobody takes it for
    covered there); it is the refine pdf at n = 1024, with mass past knot 960, that catches it."""
    c = S.cdf_case(1024, False)
    k = c["kept"] & ~c["zero_pdf"]
    u = S.u_per_ray(64, 64)[k]
    ref, bar, cmp_ = S.sample_bars(f64(c["z"])[k], c["cdf"][k], u, c["bar"][k])
    emu = S.cdf_emulation(c["z"], c["sdf"], c["beta"], False)[k]
    within = lambda cdf: bool(((f64(O._inverse_cdf(c["z"][k], cdf, u)) - ref).abs() <= bar)[cmp_].all())
    assert within(emu)
    bad = emu.clone()
    bad[:, 640:] -= (emu[:, 640] - emu[:, 320])[:, None]          # wave 2 of PER = 5 (knots from 640 on) without wave 1's total
    assert not within(bad)
    tail = emu.clone()
    tail[:, 960:] -= (emu[:, 960] - emu[:, 640])[:, None]         # wave 3 without wave 2's total
    assert within(tail)
    # ... but the refine pdf of the same rays has mass past knot 960 (the error bound grows along the ray): there the same defect is caught
    c = S.cdf_case(1024, True)
    k = c["kept"] & ~c["zero_pdf"]
    emu = S.cdf_emulation(c["z"], c["sdf"], c["beta"], True)[k]
    tail = emu.clone()
    tail[:, 960:] -= (emu[:, 960] - emu[:, 640])[:, None]
    for u in (S.u_shared(64), S.u_per_ray(64, 64).sort(-1)[0][k]):
        ref, bar, cmp_ = S.sample_bars(f64(c["z"])[k], c["cdf"][k], u, c["bar"][k])
        within = lambda cdf: bool(((f64(O._inverse_cdf(c["z"][k], cdf, u.expand(emu.shape[0], -1).contiguous())) - ref).abs() <= bar)[cmp_].all())
        assert within(emu) and not within(tail)
