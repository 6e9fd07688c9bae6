"""The depth-sampler kernels of neat_amd/csrc/kernels_sampler.hpp against float64 (tests/sampler_f64.py) at their size edges.

Which template arm and branch each size reaches (BOUND_T = 256 threads own PER consecutive intervals; the bound switches on m = n - 1,
the CDF on n):

    n               error_bound_t<PER>   resample_cdf_t<PER>
    2, 3, 65, 256   1                    1          (n = 2: m = 1, min(j0 + k, m - 1) clamps every lane onto interval 0)
    257             1                    3          (both in one launch of sampler_round_kernel)
    258, 768        3                    3
    769             3                    5          (both in one launch of sampler_round_kernel)
    770, 960, 1024  5                    5          (1024 = SMAX; n = 1024 with N = 64: the merged row of 1088 lives in global memory only)

    sample_pdf_kernel (64-bin chunks, m = nb - 1 bins): nb = 2, 3, 64 one chunk, m < 64; nb = 65 one full chunk; nb = 66 the first
      carry (one bin in chunk 2); nb = 129 two full chunks; nb = 1024 sixteen chunks.
    sampler_init_kernel: R = 1, 3, 5, 257 leave waves of the last four-ray workgroup without a ray, R = 4 fills it; picks with
      (n_step, n_cand) = (37, 5): one pick_part, grids of 37 .. 185 keys (no multiple of 4 among the odd ones: the float4 reads run into
      the +inf padding); (128, 8): four pick_parts, grids up to 1024; (257, 3): four pick_parts of which grid 257 uses two.  The keys'
      equal groups lie below every other key (sampler_f64.keys_with_ties), so they are among the 32 picks of every grid, and every grid
      of more than 256 keys picks a pair from two different parts (asserted in tests/test_sampler_math.py).
    sampler_finish_kernel: M = N + 2 + n_extra = 2, 3 (less than a wave), 64, 65 (one | two trips), 1024 (= SMAX).

What is compared how (every bar is derived or carries its measurement in tests/sampler_f64.py):
  * neat_sampler_bound: the merged sdf exactly; beta bit for bit on the rays whose bisection keeps a margin of TAU from eps at every
    evaluation (float64 reference), beta in [beta0, beta_in] on every ray; the flag.
  * neat_sampler_resample: samples within K_EMUL x (forward error bound of the ray's CDF) x (slope of the bin) + 4 ulp of 6 on the
    rays whose bound is below the cap; merge and order exactly on every ray, from the kernel's own samples.
  * neat_sampler_round: bit-identical to bound + resample; x_fm, control words and untouched outputs exactly.
  * neat_sample_pdf: samples within 4 u x slope + 4 ulp of 6; the union exactly.
  * init, finish, picks, uniform depths: exactly (the per-ray initial beta: n 2^-24 relative, float32 squares summed by a wave).
NEAT_F64_TABLE=<path> writes every measured error and left-out share as JSON lines (tests/f64_table.py).

Measured on MI355X (worst over the cases; samples: error / bar, where a bar is at least 4 ulp of 6 = 1.9e-6):
    beta, kept rays                          bit-equal at every size, plain and merged, iters 0 | 1 | 10 (0 of 48 cases with a mismatch)
    rays inside the bisection margin         0 .. 12.5 % (n = 65); allowed 25 %
    resample samples, refine | final         0.21 | 0.21 bars (n = 2; 0.04 .. 0.2 at the other sizes)
    resample samples left out                0 .. 2.4 % (n = 1024: u = 0 and u = 1 of the shared u, whose end bins fall under the rule)
    sample_pdf samples, dense | zeros        0.22 | 0.21 bars; left out at most 1.1 %
    initial beta (relative)                  at most 1.1e-7 = 1.8 x 2^-24, reached at n = 2 where the bar is 2 x 2^-24
Everything else is compared exactly.  No kernel had to change: every arm above computes what the float64 reference computes.
"""
import ctypes

import pytest
import torch

from tests import sampler_f64 as S
from tests.f64_table import record, write_table  # noqa: F401  (write_table: the NEAT_F64_TABLE writer, autouse)
from tests.sampler_f64 import F32, U, f64

pytestmark = pytest.mark.gpu
POISON = -777.25
IPOISON = -77777
K_ROUNDS = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from neat_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name, *args):
    """The C entry point itself (tensors as pointers) -> its return code."""
    from neat_amd import _lib
    fn = getattr(_lib.lib(), name)
    code = fn(*[_p(a) if isinstance(a, torch.Tensor) else a for a in args], _stream())
    torch.cuda.synchronize()
    return code


def fpoison(*shape, dev):
    return torch.full(shape, POISON, device=dev)


def ipoison(*shape, dev):
    return torch.full(shape, IPOISON, device=dev, dtype=torch.int32)


def untouched(*ts):
    return all(bool((t == (POISON if t.dtype == F32 else IPOISON)).all()) for t in ts)


def same_bits(a, b):
    """Equal bit for bit where finite or infinite; NaN where the other is NaN."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape:
        return False
    if a.dtype != F32:
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


def beta0_t(dev):
    return torch.tensor([S.BETA0], device=dev)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. neat_sampler_bound
# ------------------------------------------------------------------------------------------------------------------------------------
BOUND_CASES = [(n, N) for n in S.SIZES for N in (None, 1, 64) if N is None or n - N >= 1]


def run_bound(c, dev, iters=S.ITERS):
    from neat_amd import ops
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    so = c["sdf_old"].to(dev) if c["order"] is not None else None
    order = c["order"].to(dev) if c["order"] is not None else None
    sdf_out, beta_out = ops.sampler_bound(c["z"].to(dev), so, c["sdf_new"].to(dev), order, c["beta_in"].to(dev), beta0_t(dev), S.EPS, iters, flag)
    torch.cuda.synchronize()
    return sdf_out.cpu(), beta_out.cpu(), int(flag.item())


@pytest.mark.parametrize("n,N", BOUND_CASES)
def test_bound_beta_bit_equal_on_rays_with_a_margin(dev, n, N):
    iters_list = (S.ITERS, 0, 1) if N is None else (S.ITERS,)
    for iters in iters_list:
        c = S.bound_case(n, N, iters=iters)
        S.assert_bound_conditions(c)
        sdf_out, beta_out, flag = run_bound(c, dev, iters)
        assert torch.equal(sdf_out, c["sdf"]), "merged sdf is not the gather"
        kept = c["kept"]
        record("kernel", f"sampler_bound:left_out:N={N}:iters={iters}", n, float((~kept).float().mean()))
        wrong = int((beta_out[kept] != c["beta"][kept]).sum())
        record("kernel", f"sampler_bound:beta_mismatch:N={N}:iters={iters}", n, wrong)
        assert wrong == 0, f"n={n} N={N} iters={iters}: {wrong} of {int(kept.sum())} kept rays differ from the float64 bisection"
        b0 = torch.tensor(S.BETA0, dtype=F32)
        assert bool((beta_out >= b0).all()) and bool((beta_out <= torch.maximum(c["beta_in"], b0)).all())
        assert flag == int(bool((beta_out > b0).any())) == 1


@pytest.mark.parametrize("n", [2, 257, 1024])
def test_bound_flag(dev, n):
    """0 for a batch of closed rays only; 1 when the only open ray is the last one."""
    c = S.bound_case(n)
    closed = (c["kept"] & ~c["open"]).nonzero().flatten()
    one_open = (c["kept"] & c["open"]).nonzero().flatten()[:1]
    for rows, want in ((closed, 0), (torch.cat([closed, one_open]), 1)):
        sub = {k: (v[rows] if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
        _, beta_out, flag = run_bound(sub, dev)
        assert torch.equal(beta_out, c["beta"][rows]) and flag == want


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. neat_sampler_resample
# ------------------------------------------------------------------------------------------------------------------------------------
RESAMPLE_U = [(1, "shared"), (2, "shared"), (64, "shared"), (65, "shared"), (257, "shared"), (64, "per_ray")]


def u_for(R, N, kind, refine):
    if kind == "shared":
        return S.u_shared(N)
    u = S.u_per_ray(R, N)
    return u.sort(-1)[0] if refine else u          # the merge of a refining round takes increasing u (sorted samples)


def check_merge(z, smp, zm, order, what):
    """order is a permutation, z_merged the gather, and both equal the stable sort on finite rows (old first on ties)."""
    R, n = z.shape
    tot = n + smp.shape[1]
    cat = torch.cat([z, smp], -1)
    order = order.long()
    assert torch.equal(order.sort(-1)[0], torch.arange(tot)[None].expand(R, -1)), f"{what}: order is no permutation"
    assert same_bits(zm, cat.gather(1, order)), f"{what}: z_merged is not the gather"
    fin = torch.isfinite(smp).all(-1)
    want, worder = torch.sort(cat[fin], dim=-1, stable=True)
    assert torch.equal(zm[fin], want) and torch.equal(order[fin], worder), f"{what}: not the stable sort"


def compare_samples(entry, n, c, u, got, tally):
    k = c["kept"] & ~c["zero_pdf"]
    ref, bar, cmp_ = S.sample_bars(f64(c["z"])[k], c["cdf"][k], u if u.dim() == 1 else u[k], c["bar"][k])
    g = f64(got)[k]
    assert bool(torch.isfinite(g).all()), f"{entry} n={n}: non-finite samples on compared rays"
    ratio = float(((g - ref).abs() / bar)[cmp_].max()) if cmp_.any() else 0.0
    record("kernel", entry, n, ratio)
    tally[0] += int((~cmp_).sum())
    tally[1] += cmp_.numel()
    assert ratio <= 1.0, f"{entry} n={n}: a sample is {ratio:.2f} bars from the float64 reference"


@pytest.mark.parametrize("refine", [True, False])
@pytest.mark.parametrize("n", S.SIZES)
def test_resample_samples_and_merge(dev, n, refine):
    from neat_amd import ops
    c = S.cdf_case(n, refine)
    S.assert_cdf_conditions(c)
    R = c["z"].shape[0]
    z, sdf, beta = c["z"].to(dev), c["sdf"].to(dev), c["beta"].to(dev)
    tally = [0, 0]
    mode = "refine" if refine else "final"
    for N, kind in RESAMPLE_U:
        u = u_for(R, N, kind, refine)
        smp, zm, order = ops.sampler_resample(z, sdf, beta, u.to(dev), refine)
        torch.cuda.synchronize()
        smp = smp.cpu()
        compare_samples(f"sampler_resample:{mode}:N={N}:{kind}", n, c, u, smp, tally)
        if refine:
            check_merge(c["z"], smp, zm.cpu(), order.cpu(), f"n={n} N={N} {kind}")
        else:
            assert bool(torch.isfinite(smp).all())
            if kind == "shared":        # every knot of the final pdf is positive (pdf >= 1e-5): u = 0 lands in bin 0 with t = 0 exactly
                assert torch.equal(smp[:, 0], c["z"][:, 0])
    record("kernel", f"sampler_resample:{mode}:left_out", n, tally[0] / tally[1])
    assert tally[0] <= 0.1 * tally[1], f"{tally[0]} of {tally[1]} samples left out"


def test_resample_add_tiny_on_zero_pdf_rays(dev):
    """n = 2: rays whose refine pdf underflows draw NaN without add_tiny and the reference's samples with it."""
    from neat_amd import ops
    tiny = 1e-6
    c0, c = S.cdf_case(2, True), S.cdf_case(2, True, add_tiny=tiny)
    zero = c0["zero_pdf"]
    assert bool(zero.any()) and bool((c["kept"] & zero).any())
    u = S.u_shared(64)
    z, sdf, beta = c["z"].to(dev), c["sdf"].to(dev), c["beta"].to(dev)
    smp, zm, order = ops.sampler_resample(z, sdf, beta, u.to(dev), True, add_tiny=tiny)
    torch.cuda.synchronize()
    smp = smp.cpu()
    assert bool(torch.isfinite(smp[c["kept"]]).all())
    tally = [0, 0]
    compare_samples("sampler_resample:refine:add_tiny", 2, c, u, smp, tally)
    check_merge(c["z"], smp, zm.cpu(), order.cpu(), "add_tiny")
    smp0, zm0, order0 = ops.sampler_resample(z, sdf, beta, u.to(dev), True)
    torch.cuda.synchronize()
    check_merge(c["z"], smp0.cpu(), zm0.cpu(), order0.cpu(), "zero pdf")        # NaN samples rank above every depth


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. neat_sampler_round
# ------------------------------------------------------------------------------------------------------------------------------------
ROUND_N = [2, 257, 769, 960]
N_REFINE, N_FINAL = 64, 64


def round_inputs(n, dev):
    c = S.bound_case(n, 1 if n == 2 else 64)
    R = c["z"].shape[0]
    g = S.gen(n)
    origins = torch.randn(R, 3, generator=g)
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    return c, origins, dirs, S.u_shared(N_REFINE), S.u_per_ray(R, N_FINAL)


def round_call(c, origins, dirs, u_ref, u_fin, ctl, rnd, dev, n_refine=N_REFINE, add_tiny=0.0):
    R, n = c["z"].shape
    ldp = R * n_refine + 40
    o = {"sdf": fpoison(R, n, dev=dev), "beta": fpoison(R, dev=dev), "smp": fpoison(R, n_refine, dev=dev), "zm": fpoison(R, n + n_refine, dev=dev),
         "order": ipoison(R, n + n_refine, dev=dev), "x_fm": fpoison(3, ldp, dev=dev), "fin": fpoison(R, N_FINAL, dev=dev),
         "z_final": fpoison(R, S.SMAX, dev=dev)}
    t = [x.to(dev) for x in (c["z"], c["sdf_old"], c["sdf_new"], c["order"], c["beta_in"], u_ref, origins, dirs, u_fin)]
    code = call("neat_sampler_round", t[0], n, R, t[1], t[2], t[3], c["sdf_old"].shape[1], t[4], beta0_t(dev), S.EPS, S.ITERS, o["sdf"], o["beta"],
                ctl, rnd, K_ROUNDS, add_tiny, t[5], n_refine, o["smp"], o["zm"], o["order"], t[6], t[7], o["x_fm"], ldp, t[8], N_FINAL, N_FINAL,
                o["fin"], o["z_final"], S.SMAX)
    return code, {k: v.cpu() for k, v in o.items()}, ldp


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("n", ROUND_N)
def test_round_equals_bound_then_resample(dev, n, last):
    from neat_amd import ops
    c, origins, dirs, u_ref, u_fin = round_inputs(n, dev)
    R = c["z"].shape[0]
    rnd = K_ROUNDS - 1 if last else 0
    ctl = torch.zeros(2 * K_ROUNDS + 1, dtype=torch.int32, device=dev)
    if last:
        ctl[rnd - 1] = 1
    before = ctl.cpu().clone()
    code, o, ldp = round_call(c, origins, dirs, u_ref, u_fin, ctl, rnd, dev)
    assert code == 0
    sdf_b, beta_b, _ = run_bound(c, dev)
    assert torch.equal(o["sdf"], sdf_b) and torch.equal(o["sdf"], c["sdf"]) and torch.equal(o["beta"], beta_b)
    assert torch.equal(beta_b[c["kept"]], c["beta"][c["kept"]])
    opn = beta_b > torch.tensor(S.BETA0, dtype=F32)
    z, sdf_d, beta_d = c["z"].to(dev), sdf_b.to(dev), beta_b.to(dev)
    fin_s, _, _ = ops.sampler_resample(z, sdf_d, beta_d, u_fin.to(dev), False)
    fin_s = fin_s.cpu()
    want_ctl = before.clone()
    want_ctl[rnd] = int(bool(opn.any()))
    want_ctl[K_ROUNDS + rnd] = 1
    finalising = torch.ones_like(opn) if last else ~opn
    if bool(finalising.any()):
        want_ctl[2 * K_ROUNDS] = n
    assert torch.equal(ctl.cpu(), want_ctl), (ctl.cpu().tolist(), want_ctl.tolist())
    assert bool(opn.any()) and bool((~opn).any())
    # final samples and the final grid: the rays that finalise, nothing else
    assert same_bits(o["fin"][finalising], fin_s[finalising]) and untouched(o["fin"][~finalising])
    assert torch.equal(o["z_final"][finalising][:, :n], c["z"][finalising]) and untouched(o["z_final"][finalising][:, n:], o["z_final"][~finalising])
    if last:
        assert untouched(o["smp"], o["zm"], o["order"], o["x_fm"])
        return
    smp, zm, order = (t.cpu() for t in ops.sampler_resample(z, sdf_d, beta_d, u_ref.to(dev), True))
    assert same_bits(o["smp"], smp) and same_bits(o["zm"], zm) and torch.equal(o["order"], order)
    check_merge(c["z"], o["smp"], o["zm"], o["order"], f"round n={n}")
    assert same_bits(o["x_fm"], S.x_fm_reference(origins, dirs, o["smp"], ldp)), "x_fm is not o + (z d) / its padding is not zero"


def test_round_after_a_closed_round_writes_nothing(dev):
    c, origins, dirs, u_ref, u_fin = round_inputs(257, dev)
    ctl = torch.zeros(2 * K_ROUNDS + 1, dtype=torch.int32, device=dev)
    code, o, _ = round_call(c, origins, dirs, u_ref, u_fin, ctl, 1, dev)
    assert code == 0 and untouched(*o.values()) and not bool(ctl.any())


def test_round_of_open_rays_only_finalises_nothing(dev):
    """A round before the last in which no ray has reached beta0: no final samples, no final grid, n_final not written."""
    c, origins, dirs, u_ref, u_fin = round_inputs(769, dev)
    rows = (c["kept"] & c["open"]).nonzero().flatten()
    sub = {k: (v[rows] if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    ctl = torch.zeros(2 * K_ROUNDS + 1, dtype=torch.int32, device=dev)
    code, o, _ = round_call(sub, origins[rows], dirs[rows], u_ref, u_fin[rows], ctl, 0, dev)
    assert code == 0 and torch.equal(o["beta"], c["beta"][rows])
    assert ctl.cpu().tolist() == [1, 0, 0, 1, 0, 0, 0] and untouched(o["fin"], o["z_final"])
    assert bool(torch.isfinite(o["smp"]).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. neat_sample_pdf
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,N,zeros", S.PDF_CASES)
def test_sample_pdf_samples_and_union(dev, nb, N, zeros):
    from neat_amd import ops
    bins, w = S.pdf_inputs(nb, zeros=zeros)
    R = bins.shape[0]
    kind = "zeros" if zeros else "dense"
    for u, uk in ((S.u_shared(N), "shared"), (S.u_per_ray(R, N), "per_ray")):
        ref, bar, cmp_, den = S.pdf_reference(bins, w, u)
        if zeros:
            assert bool((f64(w).sum(-1) >= 1.5).all()) and bool((w == 0).any()) and S.rule_margin(den) >= 1.0 / 3.0
        smp, _ = ops.sample_pdf(bins.to(dev), w.to(dev), u.to(dev))
        torch.cuda.synchronize()
        smp = smp.cpu()
        assert bool(torch.isfinite(smp).all())
        ratio = float(((f64(smp) - ref).abs() / bar)[cmp_].max())
        record("kernel", f"sample_pdf:{kind}:N={N}:{uk}", nb, ratio)
        record("kernel", f"sample_pdf:{kind}:N={N}:{uk}:left_out", nb, float((~cmp_).float().mean()))
        assert ratio <= 1.0, f"nb={nb} N={N} {kind} {uk}: a sample is {ratio:.2f} bars from the float64 reference"
        assert float((~cmp_).float().mean()) <= 0.1
    g = S.gen(nb + N)
    u = S.u_per_ray(R, N)
    for nz in sorted({1, nb + 1, S.SMAX - N if (nb, N) == (129, 65) else 1}):
        if nz + N > S.SMAX:
            continue
        zmerge = torch.rand(R, nz, generator=g) * 6
        zmerge[:, 0] = bins[:, 0]                  # u = 0-like ties with the first bin edge
        smp, union = ops.sample_pdf(bins.to(dev), w.to(dev), u.to(dev), z_merge=zmerge.to(dev))
        torch.cuda.synchronize()
        smp, union = smp.cpu(), union.cpu()
        assert torch.equal(union, torch.sort(torch.cat([zmerge, smp], -1), -1)[0]), f"nb={nb} N={N} nz={nz}: union is not the sort"


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. neat_sampler_init / neat_sampler_init_rays
# ------------------------------------------------------------------------------------------------------------------------------------
INIT_R, INIT_N, INIT_NCTL = (1, 3, 4, 5, 257), (2, 64, 65, 129, 1024), (0, 11, 257)
INIT_PICKS = ((37, 5), (128, 8), (257, 3))
INIT_CASES = [(R, n, INIT_NCTL[(i + j) % 3], INIT_PICKS[(i + 2 * j) % 3]) for i, R in enumerate(INIT_R) for j, n in enumerate(INIT_N)]
N_EXTRA = 32


@pytest.mark.parametrize("R,n,nctl,picks", INIT_CASES)
def test_init(dev, R, n, nctl, picks):
    n_step, n_cand = picks
    z, _ = S.rays(n, R=R, seed=3)
    g = S.gen(R * 2000 + n)
    origins = torch.randn(R, 3, generator=g)
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    keys = S.keys_with_ties(n_step * n_cand)
    beta_param, beta_min = -0.0137, 1e-4
    want_beta0, want_beta = S.init_reference(z, beta_param, beta_min)
    ldp = R * n + 24
    bp = torch.tensor([beta_param], device=dev)
    zd = z.to(dev)

    def outputs():
        return fpoison(1, dev=dev), fpoison(R, dev=dev), ipoison(nctl + 4, dev=dev)

    def check_common(beta0, beta, ctl, what):
        assert torch.equal(beta0.cpu(), want_beta0.reshape(1)), what
        err = float(((f64(beta) - want_beta).abs() / want_beta).max())
        record("kernel", f"{what}:beta", (R, n), err)
        assert err <= n * U, f"{what} R={R} n={n}: beta err {err:.2e} > n 2^-24"
        assert not bool(ctl[:nctl].any()) and untouched(ctl[nctl:]), f"{what}: ctl"

    beta0, beta, ctl = outputs()
    assert call("neat_sampler_init", zd, R, n, bp, beta_min, S.beta_c(), beta0, beta, ctl, nctl) == 0
    check_common(beta0, beta, ctl, "sampler_init")

    beta0, beta, ctl = outputs()
    x_fm, pick_all = fpoison(3, ldp, dev=dev), ipoison(n_cand, N_EXTRA, dev=dev)
    assert call("neat_sampler_init_rays", zd, R, n, bp, beta_min, S.beta_c(), beta0, beta, ctl, nctl, origins.to(dev), dirs.to(dev), x_fm, ldp,
                keys.to(dev), n_step, n_cand, N_EXTRA, pick_all) == 0
    check_common(beta0, beta, ctl, "sampler_init_rays")
    assert same_bits(x_fm, S.x_fm_reference(origins, dirs, z, ldp)), "x_fm is not o + (z d) / its padding is not zero"
    pick_all = pick_all.cpu().long()
    for c in range(n_cand):
        assert torch.equal(pick_all[c], S.picks_reference(keys, n_step * (c + 1), N_EXTRA)), f"picks of grid {n_step * (c + 1)}"


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. neat_sampler_finish, neat_sampler_finish_dev, neat_sampler_finish_picked
# ------------------------------------------------------------------------------------------------------------------------------------
FINISH_CASES = [(0, 0), (1, 0), (30, 32), (31, 32), (990, 32), (510, 512)]          # (N, n_extra): M = 2, 3, 64, 65, 1024, 1024
FIN_R, FIN_n, NEAR, FAR = 5, 129, 0.25, 5.5


def finish_inputs(N, n_extra, dev, n=FIN_n):
    g = S.gen(100 * N + n_extra)
    M = N + 2 + n_extra
    grid = (torch.rand(FIN_R, n, generator=g) * 6).sort(-1)[0]
    zf = torch.full((FIN_R, n + 5), POISON)
    zf[:, :n] = grid
    smp = (torch.rand(FIN_R, max(N, 1), generator=g) * 6).sort(-1)[0]
    if N >= 3:                                      # ties: near, far, and a picked depth among the samples
        smp[:, 0], smp[:, 1], smp[:, 2] = NEAR, FAR, grid[:, 0]
    eik = torch.randint(M, (FIN_R,), generator=g, dtype=torch.int32)
    eik[0], eik[-1] = 0, M - 1
    return grid, zf, smp, eik, M


def check_finish(what, out, zeik, smp, N, grid, pick, eik, M):
    rows = S.finish_reference(smp[:, :N], grid, pick, NEAR, FAR)
    assert rows.shape == (FIN_R, M)
    out, zeik = out.cpu(), zeik.cpu()
    assert torch.equal(out, torch.sort(rows, -1)[0]) and torch.equal(out, rows), f"{what}: rows are not the sort of the gathered row"
    assert torch.equal(zeik.flatten(), out.gather(1, eik.long()[:, None]).flatten()), f"{what}: z_eik"


@pytest.mark.parametrize("N,n_extra", FINISH_CASES + [(0, 1)])
def test_finish_host_picks(dev, N, n_extra):
    grid, zf, smp, eik, M = finish_inputs(N, n_extra, dev)
    pick = torch.randint(FIN_n, (max(n_extra, 1),), generator=S.gen(N), dtype=torch.int32)
    pick[0] = 0                                     # grid[:, 0] is among the samples
    if n_extra >= 4:
        pick[1], pick[2], pick[3] = FIN_n - 1, pick[0], FIN_n - 1          # repeated picks
    out, zeik = fpoison(FIN_R, M, dev=dev), fpoison(FIN_R, dev=dev)
    gd = grid.to(dev)
    assert call("neat_sampler_finish", smp.to(dev), N, gd, FIN_n, pick.to(dev), n_extra, NEAR, FAR, FIN_R, eik.to(dev), out, zeik) == 0
    check_finish("finish", out, zeik, smp, N, grid, pick[:n_extra], eik, M)


@pytest.mark.parametrize("N,n_extra", FINISH_CASES)
def test_finish_device_picks(dev, N, n_extra):
    """finish_picked (pick_all row n / n_step - 1), finish_dev with keys (the n_extra smallest) and without (the eval formula)."""
    grid, zf, smp, eik, M = finish_inputs(N, n_extra, dev)
    n_final = torch.tensor([FIN_n], dtype=torch.int32, device=dev)
    zfd, sd, ed = zf.to(dev), smp.to(dev), eik.to(dev)
    ld = zf.shape[1]
    n_step, n_cand = 43, 4                          # 129 / 43 - 1 = row 2
    pick_all = torch.randint(43, (n_cand, max(n_extra, 1)), generator=S.gen(7 + N), dtype=torch.int32)
    pick_all[2] = torch.randint(FIN_n, (max(n_extra, 1),), generator=S.gen(8 + N), dtype=torch.int32)
    if n_extra >= 4:
        pick_all[2, :4] = torch.tensor([0, FIN_n - 1, 0, FIN_n - 1])
    out, zeik = fpoison(FIN_R, M, dev=dev), fpoison(FIN_R, dev=dev)
    assert call("neat_sampler_finish_picked", sd, N, zfd, ld, n_final, pick_all.to(dev), n_step, n_extra, NEAR, FAR, FIN_R, ed, out, zeik) == 0
    check_finish("finish_picked", out, zeik, smp, N, grid, pick_all[2, :n_extra], eik, M)
    if n_extra <= FIN_n:
        keys = S.keys_with_ties(FIN_n, seed=N)
        out, zeik, pick = fpoison(FIN_R, M, dev=dev), fpoison(FIN_R, dev=dev), ipoison(max(n_extra, 1), dev=dev)
        assert call("neat_sampler_finish_dev", sd, N, zfd, ld, n_final, keys.to(dev), n_extra, pick, NEAR, FAR, FIN_R, ed, out, zeik) == 0
        want = S.picks_reference(keys, FIN_n, n_extra)
        assert torch.equal(pick.cpu().long()[:n_extra], want)
        check_finish("finish_dev keys", out, zeik, smp, N, grid, want, eik, M)
    out, zeik, pick = fpoison(FIN_R, M, dev=dev), fpoison(FIN_R, dev=dev), ipoison(max(n_extra, 1), dev=dev)
    assert call("neat_sampler_finish_dev", sd, N, zfd, ld, n_final, None, n_extra, pick, NEAR, FAR, FIN_R, ed, out, zeik) == 0
    want = S.eval_pick(FIN_n, n_extra) if n_extra else torch.zeros(0, dtype=torch.long)
    assert torch.equal(pick.cpu().long()[:n_extra], want)
    check_finish("finish_dev eval", out, zeik, smp, N, grid, want, eik, M)
    out, zeik = fpoison(FIN_R, M, dev=dev), fpoison(FIN_R, dev=dev)          # finish_picked without pick_all: the formula inside the finish kernel
    assert call("neat_sampler_finish_picked", sd, N, zfd, ld, n_final, None, n_step, n_extra, NEAR, FAR, FIN_R, ed, out, zeik) == 0
    check_finish("finish_picked eval", out, zeik, smp, N, grid, want, eik, M)


def test_eval_pick_formula_and_device_key_picks(dev):
    """torch.linspace(0, n - 1, n_extra).long() at sizes other than 128 k; the one-workgroup key picks at n = 37, 257, 1023."""
    R, N = 2, 1
    zf = (torch.rand(R, S.SMAX, generator=S.gen(1)) * 6).sort(-1)[0].to(dev)
    smp, eik = torch.full((R, N), 3.0, device=dev), torch.zeros(R, dtype=torch.int32, device=dev)
    for n in (2, 3, 127, 129, 1023, 1024):
        n_final = torch.tensor([n], dtype=torch.int32, device=dev)
        for n_extra in (2, 3, 32, 33):
            M = N + 2 + n_extra
            out, zeik, pick = fpoison(R, M, dev=dev), fpoison(R, dev=dev), ipoison(n_extra, dev=dev)
            assert call("neat_sampler_finish_dev", smp, N, zf, S.SMAX, n_final, None, n_extra, pick, NEAR, FAR, R, eik, out, zeik) == 0
            assert torch.equal(pick.cpu().long(), S.eval_pick(n, n_extra)), (n, n_extra, pick.tolist())
            rows = S.finish_reference(smp.cpu(), zf.cpu(), S.eval_pick(n, n_extra), NEAR, FAR)
            assert torch.equal(out.cpu(), rows)
            out2, zeik2 = fpoison(R, M, dev=dev), fpoison(R, dev=dev)
            assert call("neat_sampler_finish_picked", smp, N, zf, S.SMAX, n_final, None, 1, n_extra, NEAR, FAR, R, eik, out2, zeik2) == 0
            assert torch.equal(out2, out) and torch.equal(zeik2, zeik)
    for n in (37, 257, 1023):
        keys = S.keys_with_ties(n, seed=1)
        n_final = torch.tensor([n], dtype=torch.int32, device=dev)
        out, zeik, pick = fpoison(R, N + 2 + 32, dev=dev), fpoison(R, dev=dev), ipoison(32, dev=dev)
        assert call("neat_sampler_finish_dev", smp, N, zf, S.SMAX, n_final, keys.to(dev), 32, pick, NEAR, FAR, R, eik, out, zeik) == 0
        assert torch.equal(pick.cpu().long(), S.picks_reference(keys, n, 32)), n


# ------------------------------------------------------------------------------------------------------------------------------------
# 7. neat_uniform_depths
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("N", [1, 2, 257])
def test_uniform_depths(dev, N, R):
    """Bit-equal to the reference's chain of elementwise float32 operations, plain and jittered, per-ray near and far."""
    from neat_amd import ops
    g = S.gen(10 * N + R)
    near, far = torch.rand(R, 1, generator=g), torch.rand(R, 1, generator=g) * 4 + 1.5
    rnd = torch.rand(R, N, generator=g)
    t = torch.linspace(0.0, 1.0, N)
    for nr, fr in ((near, far), (0.5, far), (near, 6.0), (0.0, 6.0)):
        nt = nr if isinstance(nr, torch.Tensor) else torch.full((R, 1), nr)
        ft = fr if isinstance(fr, torch.Tensor) else torch.full((R, 1), fr)
        z0 = nt * (1.0 - t) + ft * t
        mid = 0.5 * (z0[:, 1:] + z0[:, :-1])
        hi, lo = torch.cat([mid, z0[:, -1:]], -1), torch.cat([z0[:, :1], mid], -1)
        z1 = lo + (hi - lo) * rnd
        nd = nr.to(dev) if isinstance(nr, torch.Tensor) else nr
        fd = fr.to(dev) if isinstance(fr, torch.Tensor) else fr
        assert torch.equal(ops.uniform_depths(R, N, nd, fd, None, dev).cpu(), z0)
        assert torch.equal(ops.uniform_depths(R, N, nd, fd, rnd.to(dev), dev).cpu(), z1)
        if isinstance(nr, float) and isinstance(fr, float):
            assert torch.equal(z0, S.O.uniform_z(R, N, nr, fr)) and torch.equal(z1, S.O.uniform_z(R, N, nr, fr, rnd))


# ------------------------------------------------------------------------------------------------------------------------------------
# 8. refusals: an error code before any launch, the outputs untouched
# ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from neat_amd import ops
    R, big = 2, S.SMAX + 8
    f = lambda *s: torch.zeros(*s, device=dev)
    i32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.int32)
    u64 = torch.linspace(0, 1, 64, device=dev)
    for n in (1, S.SMAX + 1):
        outs = [fpoison(R, big, dev=dev), fpoison(R, dev=dev), ipoison(1, dev=dev)]
        assert call("neat_sampler_bound", f(R, big), n, R, None, f(R, big), None, 0, f(R), beta0_t(dev), S.EPS, S.ITERS, *outs) != 0
        assert untouched(*outs)
        outs = [fpoison(R, 64, dev=dev), fpoison(R, 2 * big, dev=dev), ipoison(R, 2 * big, dev=dev)]
        assert call("neat_sampler_resample", f(R, big), f(R, big), n, R, f(R) + 0.1, 1, 0.0, u64, 0, 64, *outs) != 0
        assert untouched(*outs)
        outs = [fpoison(1, dev=dev), fpoison(R, dev=dev), ipoison(8, dev=dev)]
        assert call("neat_sampler_init", f(R, big), R, n, f(1) + 0.1, 1e-4, S.beta_c(), *outs, 8) != 0
        assert untouched(*outs)
        with pytest.raises(RuntimeError):
            ops.sampler_resample(f(R, n), f(R, n), f(R) + 0.1, u64, True)
    # neat_sampler_round: n = 1, n = 1025, and n + N_refine = 1025 in a round that refines
    for n, n_refine, rnd in ((1, 64, 0), (S.SMAX + 1, 64, 0), (S.SMAX + 1, 64, K_ROUNDS - 1), (961, 64, 0), (S.SMAX, 1, 0)):
        o = [fpoison(R, big, dev=dev), fpoison(R, dev=dev), ipoison(2 * K_ROUNDS + 1, dev=dev), fpoison(R, 64, dev=dev), fpoison(R, 2 * big, dev=dev),
             ipoison(R, 2 * big, dev=dev), fpoison(3, R * 64 + 8, dev=dev), fpoison(R, 64, dev=dev), fpoison(R, big, dev=dev)]
        code = call("neat_sampler_round", f(R, big), n, R, None, f(R, big), None, 0, f(R) + 0.1, beta0_t(dev), S.EPS, S.ITERS, o[0], o[1], o[2], rnd,
                    K_ROUNDS, 0.0, u64, n_refine, o[3], o[4], o[5], f(R, 3), f(R, 3), o[6], R * 64 + 8, u64, 0, 64, o[7], o[8], big)
        assert code != 0 and untouched(*o), (n, n_refine, rnd)
    # the finishes: N + 2 + n_extra = 1025; n_extra = 1 where the device picks
    n_final = torch.tensor([129], dtype=torch.int32, device=dev)
    for N, n_extra in ((991, 32), (32, 1)):
        M = N + 2 + n_extra
        outs = [fpoison(R, M, dev=dev), fpoison(R, dev=dev)]
        if n_extra != 1:
            assert call("neat_sampler_finish", f(R, N), N, f(R, 134), 129, i32(n_extra), n_extra, NEAR, FAR, R, i32(R), *outs) != 0
        pick = ipoison(n_extra, dev=dev)
        assert call("neat_sampler_finish_dev", f(R, N), N, f(R, 134), 134, n_final, f(129), n_extra, pick, NEAR, FAR, R, i32(R), *outs) != 0
        assert call("neat_sampler_finish_dev", f(R, N), N, f(R, 134), 134, n_final, None, n_extra, pick, NEAR, FAR, R, i32(R), *outs) != 0
        assert call("neat_sampler_finish_picked", f(R, N), N, f(R, 134), 134, n_final, i32(3, n_extra), 43, n_extra, NEAR, FAR, R, i32(R), *outs) != 0
        assert untouched(pick, *outs)
    # sample_pdf: nz + N = 1025
    outs = [fpoison(R, 64, dev=dev), fpoison(R, S.SMAX + 1, dev=dev)]
    assert call("neat_sample_pdf", f(R, 65), f(R, 64) + 1, 65, R, u64, 0, 64, outs[0], f(R, 961), 961, outs[1]) != 0
    assert untouched(*outs)
    for nb in (1, S.SMAX + 1):
        assert call("neat_sample_pdf", f(R, big), f(R, big) + 1, nb, R, u64, 0, 64, outs[0], None, 0, None) != 0
    assert untouched(*outs)
