"""Float64 references, seeded CPU inputs, margins and error bars for tests/test_f64_sampler_edges.py (the kernels of
neat_amd/csrc/kernels_sampler.hpp); tests/test_sampler_math.py checks everything here without a GPU.

References are the oracle's own functions (oracle/neat_oracle.py: _d_star, _error_bound, laplace_density, free_energy_weights,
_inverse_cdf, sample_pdf, uniform_z) run on float64 copies of the float32 inputs the kernel sees; the merge, the finish sort, the picks
and the init are a few lines of plain torch here.  Nothing in this module imports the code under test and nothing needs a GPU.

Inputs: rays through a unit sphere.  z sorted uniform in [0, 6], sdf(z) = sqrt((z - 3)^2 + h^2) - 1 with h uniform in [0, 1.5] per ray:
a true SDF along a ray; h > 1 misses the surface, h < 1 crosses it.

Three kinds of margin, all computed from the float64 reference alone:
 * bisection: the smallest |err - eps| / eps over the evaluations a ray really makes; rays below TAU are not compared bit for bit.
 * CDF knots: a first-order forward bound of the float32 formula per ray (cdf_reference); the bar of a ray is K_EMUL x bound, rays whose
   bound exceeds the cap are not compared (the formula cancels on them: 0.5 + 0.5 sign expm1(-|s| / beta), and exp(sum) - 1).
 * samples: bar = CDF bar x slope of the bin + 4 ulp of 6; samples whose bin sits at the `den < 1e-5` rule, or whose u lies within the
   CDF bar of a knot at which the inverse CDF jumps, are left out (sample_bars)."""
import math

import torch

from oracle import neat_oracle as O
from tests.f64_reference import F64, cached  # noqa: F401

F32 = torch.float32
U = 2.0 ** -24                      # unit roundoff of float32
BETA0, EPS, ITERS = 0.02, 0.1, 10
SMAX = 1024
SIZES = (2, 3, 65, 256, 257, 258, 768, 769, 770, 1024)
R_RAYS = 64
SATURATED = 17.4                    # expm1f(-x) == -1 for x >= 25 ln 2 = 17.33
ULP6 = 2.0 ** -21                   # ulp of a float32 in [4, 8): the depths reach 6

# Bisection margin.  Largest difference between the float32 and the float64 run of the oracle's _d_star + _error_bound at the betas the
# bisection visits, relative to max(err, eps), over SIZES + (960,), plain and merged from N = 1 | 64 new depths, seed 0, 64 rays:
# 5.1e-7 (n = 768) .. 1.87e-5 (n = 2, where Heron's area of the one interval cancels; 7.1e-6 with a float64 d*).  x 8: the kernel's
# bound uses the hardware exp2 / reciprocal forms (about 2 ulp each, its own comment) under an exp of a sum of up to ln 1e6 -> 1.5e-4,
# rounded up to 2e-4 so that another build of the CPU's exp and sqrt has room (tests/test_sampler_math.py asserts 8 x measured <= TAU).
TAU = 2e-4
TAU_MEASURED = 1.87e-5

# CDF bars.  A ray's knots are compared when its forward bound (cdf_reference) is at most the cap.  K_EMUL = 4 x the largest ratio
# (knot error of cdf_emulation: the kernel's arithmetic on the CPU, float32 terms, float64 prefix sums, one rounding per knot) / bound
# over the kept rays of both pdfs at SIZES + (960,): 5.2e-2 (n = 3, refine); 4e-3 .. 1.9e-2 at n >= 65
# (tests/test_sampler_math.py measures it again).
# The cap at n >= 769, measured against the float64 reference on these rays: the kept rays' bounds reach 8.3e-4 (4.4e-4 at n = 769),
# the emulation stays at <= 1.2e-2 of the bound and the kernel on MI355X at <= 0.2 bars, as below 769.  With 1e-4 only 2 % of the rays
# of the final pdf at n = 1024 would be compared.
CAP_SMALL, CAP_LARGE = 1e-4, 1e-3          # n < 769 | n >= 769
K_EMUL_MEASURED = 0.055
K_EMUL = 4 * K_EMUL_MEASURED
# sample_pdf: only the normalisation pdf / sum and the rounding of a knot contribute -> 4 u per knot
PDF_KNOT_BAR = 4 * U


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f64(t):
    return t.detach().cpu().to(F64)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def rays(n, R=R_RAYS, seed=0):
    """-> z [R,n] sorted in [0, 6], sdf [R,n] of the unit sphere along the ray, both float32 (what the kernel sees)."""
    g = gen(1000003 * seed + n)
    z = (torch.rand(R, n, generator=g) * 6).sort(-1)[0]
    h = torch.rand(R, 1, generator=g) * 1.5
    sdf = (torch.sqrt((f64(z) - 3.0) ** 2 + f64(h) ** 2) - 1.0).to(F32)
    return z, sdf


def beta_c(eps=EPS):
    """1 / (4 log(1 + eps)), the float32 constant of ray_sampler.py:139 as the oracle writes it."""
    return float(1.0 / (4.0 * torch.log(torch.tensor(eps + 1.0))))


def beta_init(z, dtype=F32):
    """The reference's initial beta sqrt(beta_c sum gap^2) per ray (oracle.error_bound_sampler's line)."""
    z = z.to(dtype)
    delta = z[:, 1:] - z[:, :-1]
    return torch.sqrt((1.0 / (4.0 * torch.log(torch.tensor(EPS + 1.0)))).to(dtype) * (delta ** 2.0).sum(-1))


def merged_case(n, N, seed=0):
    """A grid of n depths that is the stable-sorted union of n - N old and N new depths: -> z [R,n], sdf_old [R,n-N], sdf_new [R,N],
    order int32 [R,n] (index into cat[old, new]), merged sdf [R,n]."""
    z_all, sdf_all = rays(n, seed=seed + 7)
    R = z_all.shape[0]
    g = gen(31 * n + N)
    perm = torch.stack([torch.randperm(n, generator=g) for _ in range(R)])
    old_i, new_i = perm[:, :n - N].sort(-1)[0], perm[:, n - N:].sort(-1)[0]
    cat_z = torch.cat([z_all.gather(1, old_i), z_all.gather(1, new_i)], -1)
    cat_s = torch.cat([sdf_all.gather(1, old_i), sdf_all.gather(1, new_i)], -1)
    z, order = torch.sort(cat_z, dim=-1, stable=True)
    return z, cat_s[:, :n - N].contiguous(), cat_s[:, n - N:].contiguous(), order.to(torch.int32), cat_s.gather(1, order)


# ---- the beta bisection ------------------------------------------------------------------------------------------------------------
def bound_terms(z, sdf, dtype=F64):
    z, sdf = z.to(dtype), sdf.to(dtype)
    delta = z[:, 1:] - z[:, :-1]
    return sdf, delta, O._d_star(sdf, delta)


def bisect(z, sdf, beta_in, beta0=BETA0, eps=EPS, iters=ITERS, visits=None):
    """The reference's line search (oracle.error_bound_sampler) with lo / hi / mid in float32 -- (lo + hi) / 2 is exact there, as in the
    kernel -- and the bound in float64.  -> beta [R] float32, margin [R]: the smallest |err - eps| / eps over the evaluations the ray
    really makes (a ray closed at beta0 makes one).  visits (list) collects (beta [R] float32, evaluated mask) of every evaluation."""
    sdf64, delta, ds = bound_terms(z, sdf)
    R = z.shape[0]
    lo = torch.full((R,), beta0, dtype=F32)
    hi = beta_in.detach().cpu().to(F32).clone()
    err = O._error_bound(f64(lo)[:, None], sdf64, delta, ds)
    margin = (err - eps).abs() / eps
    active = err > eps
    if visits is not None:
        visits.append((lo.clone(), torch.ones(R, dtype=torch.bool)))
    hi = torch.where(active, hi, lo)
    for _ in range(iters):
        mid = (lo + hi) / 2.0
        err = O._error_bound(f64(mid)[:, None], sdf64, delta, ds)
        if visits is not None:
            visits.append((mid.clone(), active.clone()))
        margin = torch.where(active, torch.minimum(margin, (err - eps).abs() / eps), margin)
        hi = torch.where(active & (err <= eps), mid, hi)
        lo = torch.where(active & (err > eps), mid, lo)
    return hi, margin


def bound_f32_vs_f64(z, sdf, beta_in):
    """Largest relative difference of the float32 and float64 runs of _d_star + _error_bound at the betas the bisection visits."""
    visits = []
    bisect(z, sdf, beta_in, visits=visits)
    t64, t32 = bound_terms(z, sdf), bound_terms(z, sdf, F32)
    worst = 0.0
    for beta, mask in visits:
        if not mask.any():
            continue
        e64 = O._error_bound(f64(beta)[:, None], *t64)
        e32 = O._error_bound(beta[:, None], *t32)
        rel = ((f64(e32) - e64).abs() / e64.clamp_min(EPS))[mask]          # (below eps: relative to eps, what the margin is relative to)
        if rel.numel():
            worst = max(worst, float(rel.max()))
    return worst


def bound_case(n, N=None, seed=0, iters=ITERS):
    """Inputs and reference of one neat_sampler_bound case (N: merged from n - N old and N new depths).  kept: margin >= TAU."""
    def make():
        if N is None:
            z, sdf = rays(n, seed=seed)
            c = {"z": z, "sdf": sdf, "sdf_old": None, "sdf_new": sdf, "order": None}
        else:
            z, so, sn, order, sdf = merged_case(n, N, seed)
            c = {"z": z, "sdf": sdf, "sdf_old": so, "sdf_new": sn, "order": order}
        c["beta_in"] = beta_init(c["z"])
        c["beta"], c["margin"] = bisect(c["z"], c["sdf"], c["beta_in"], iters=iters)
        c["kept"] = c["margin"] >= TAU
        c["open"] = c["beta"] > BETA0
        return c
    return cached(("bound", n, N, seed, iters), make)


def assert_bound_conditions(c):
    """At most 25 % of the rays left out; at least one open and one closed ray kept."""
    kept, opn = c["kept"], c["open"]
    assert float((~kept).float().mean()) <= 0.25, f"{int((~kept).sum())} of {kept.numel()} rays inside the bisection margin"
    assert bool((kept & opn).any()) and bool((kept & ~opn).any()), "need a kept open ray and a kept closed ray"


# ---- the CDF of a resampling round -----------------------------------------------------------------------------------------------------
def _pdf(z, sdf, beta, refine, add_tiny, dtype):
    """The oracle's lines :278-293 on `dtype` copies -> pdf [R,n-1] (not normalised) and the pieces the forward bound needs."""
    z, sdf, beta = z.to(dtype), sdf.to(dtype), beta.to(dtype)[:, None]
    sigma = O.laplace_density(sdf, beta)
    w, trans, delta_full = O.free_energy_weights(z, sigma)
    delta = z[:, 1:] - z[:, :-1]
    ds = O._d_star(sdf, delta)
    if refine:
        err_sec = torch.exp(-ds / beta) * delta ** 2 / (4.0 * beta ** 2)
        pdf = (torch.clamp(torch.exp(torch.cumsum(err_sec, -1)), max=1.0e6) - 1.0) * trans[:, :-1] + add_tiny
    else:
        err_sec = None
        pdf = w[:, :-1] + 1e-5
    return pdf, {"sigma": sigma, "trans": trans, "delta": delta, "ds": ds, "err_sec": err_sec, "beta": beta, "sdf": sdf}


def _cdf_of(pdf):
    pdf = pdf / pdf.sum(-1, keepdim=True)
    return torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)


def _excl(x):
    return torch.cumsum(x, -1) - x


def cdf_reference(z, sdf, beta, refine, add_tiny=0.0):
    """-> cdf [R,n] float64 (NaN rows: pdf sums to zero), bound [R]: first-order forward error bound of the float32 formula's knots.

    u = 2^-24 is carried through the formula, every float32 operation adding u x |result| and every error passing through the
    derivative of what follows (sums run in float64 in the kernel and add nothing):
      sigma = (1 / beta)(0.5 + 0.5 sign expm1(-|s| / beta)): |d sigma| <= u (2 / beta + 3 sigma)      (the cancellation of 0.5 - 0.5 x;
                                                               past |s| / beta >= 17.4 expm1 is -1 exactly in float32 (e^-17.4 < 2^-25) and
                                                               the sum 0 or 1 exactly: no cancellation is left, only the truncation of
                                                               the float64 sigma, at most 2^-26 / beta = u / (4 beta), which replaces the
                                                               2 / beta term there.  This departs from the issue's u (2 / beta + 3 sigma)
                                                               on every knot: with that, the empty stretches of a ray carry most of the
                                                               bound and n = 768 keeps fewer than half of its rays under the 1e-4 cap)
      e = d sigma, re = exclusive prefix, T = exp(-re):       |d T| <= T (d re + u re + 2 u)             ((float) re, then expf)
      d* by Heron: area = s (s-a)(s-b)(s-c), each factor wrong by u s -> |d ds| <= ds (u / 2)(s/(s-a) + s/(s-b) + s/(s-c) + 8)
      sv = exp(-ds / beta) d^2 / (4 beta^2):                  |d sv| <= sv (d ds / beta + u ds / beta + 6 u)
      refine pdf = (min(exp rs, 1e6) - 1) T:                  |d pdf| <= E (d rs + u rs + 2 u) T + (E - 1) dT + 2 u (E T)
      final  pdf = (1 - exp(-e)) T + 1e-5:                    |d pdf| <= (exp(-e)(d e + 2 u) + u alpha) T + alpha dT + 2 u pdf
    A knot is a ratio of two sums of pdf values, each wrong by at most sum(d pdf): 2 sum(d pdf) / sum(pdf), + 4 u for the division,
    the rounding of the knot and of the normaliser."""
    pdf, p = _pdf(z, sdf, beta, refine, add_tiny, F64)
    sigma, trans, delta, beta64 = p["sigma"], p["trans"], p["delta"], p["beta"]
    live = p["sdf"].abs() / beta64 < SATURATED
    d_sigma = U * (torch.where(live, 2.0 / beta64, 0.25 / beta64) + 3.0 * sigma)
    e = delta * sigma[:, :-1]
    d_e = delta * d_sigma[:, :-1] + 2 * U * e
    re = _excl(e)
    T = trans[:, :-1]
    d_T = T * (_excl(d_e) + U * re + 2 * U)
    if refine:
        a, b, c = delta, p["sdf"][:, :-1].abs(), p["sdf"][:, 1:].abs()
        s = (a + b + c) / 2.0
        heron = (p["ds"] > 0) & ~(a * a + b * b <= c * c) & ~(a * a + c * c <= b * b)
        cond = s / (s - a).clamp_min(1e-300) + s / (s - b).clamp_min(1e-300) + s / (s - c).clamp_min(1e-300) + 8.0
        d_ds = torch.where(heron, p["ds"] * 0.5 * U * cond, torch.zeros_like(a))
        sv = p["err_sec"]
        d_sv = sv * (d_ds / beta64 + U * p["ds"] / beta64 + 6 * U)
        rs = torch.cumsum(sv, -1)
        E = torch.clamp(torch.exp(rs), max=1.0e6)
        d_pdf = E * (torch.cumsum(d_sv, -1) + U * rs + 2 * U) * T + (E - 1.0) * d_T + 2 * U * E * T
    else:
        alpha = 1.0 - torch.exp(-e)
        d_pdf = (torch.exp(-e) * (d_e + 2 * U) + U * alpha) * T + alpha * d_T + 2 * U * pdf
    total = pdf.sum(-1)
    bound = torch.where(total > 0, 2.0 * d_pdf.sum(-1) / total.clamp_min(1e-300) + 4 * U, torch.full_like(total, math.inf))
    bound = torch.where(torch.isfinite(bound), bound, torch.full_like(bound, math.inf))
    if z.shape[1] == 2:                 # one bin: its upper knot is pdf / pdf = 1 whatever the pdf's error, once the float32 pdf is not 0
        bound = torch.where(bound <= 0.5, torch.full_like(total, 4 * U), bound)
    return _cdf_of(pdf), bound


def cdf_emulation(z, sdf, beta, refine, add_tiny=0.0):
    """The kernel's arithmetic (resample_cdf_t) on the CPU: float32 terms, float64 prefix sums, one rounding per knot."""
    z, sdf, b = z.to(F32), sdf.to(F32), beta.to(F32)[:, None]
    d = z[:, 1:] - z[:, :-1]
    sigma = (1.0 / b) * (0.5 + 0.5 * sdf.sign() * torch.expm1(-sdf.abs() / b))
    e = torch.cat([d, torch.full_like(d[:, :1], 1e10)], -1) * sigma
    T = torch.exp(-(_excl(e.to(F64)).to(F32)))[:, :-1]
    if refine:
        sv = torch.exp(-O._d_star(sdf, d) / b) * (d * d) / (4.0 * b * b)
        pv = (torch.clamp(torch.exp(torch.cumsum(sv.to(F64), -1).to(F32)), max=1.0e6) - 1.0) * T + add_tiny
    else:
        pv = (1.0 - torch.exp(-e[:, :-1])) * T + 1e-5
    total = pv.to(F64).sum(-1, keepdim=True).to(F32)
    q = pv / total
    return torch.cat([torch.zeros_like(q[:, :1]), torch.cumsum(q.to(F64), -1).to(F32)], -1)


def cdf_cap(n):
    return CAP_LARGE if n >= 769 else CAP_SMALL


def cdf_case(n, refine, seed=0, add_tiny=0.0):
    """Inputs and reference of a resampling case: the rays of bound_case with the reference's beta.  kept: bound <= cap (and a pdf that
    does not sum to zero); bar [R] = K_EMUL x bound."""
    def make():
        b = bound_case(n, seed=seed)
        cdf, bound = cdf_reference(b["z"], b["sdf"], b["beta"], refine, add_tiny)
        kept = bound <= cdf_cap(n)
        return {"z": b["z"], "sdf": b["sdf"], "beta": b["beta"], "open": b["open"], "cdf": cdf, "bound": bound, "kept": kept,
                "bar": K_EMUL * bound, "zero_pdf": ~torch.isfinite(cdf).all(-1)}
    return cached(("cdf", n, bool(refine), seed, add_tiny), make)


def assert_cdf_conditions(c):
    """At least half of the rays and at least half of the open rays are compared."""
    kept, opn = c["kept"], c["open"]
    assert int(kept.sum()) * 2 >= kept.numel(), f"only {int(kept.sum())} of {kept.numel()} rays within the cap"
    assert int((kept & opn).sum()) * 2 >= int(opn.sum()), f"only {int((kept & opn).sum())} of {int(opn.sum())} open rays within the cap"


def emulation_ratio(c, refine, add_tiny=0.0):
    """Largest (knot error of the emulation) / bound over the kept rays of a case."""
    emu = f64(cdf_emulation(c["z"], c["sdf"], c["beta"], refine, add_tiny))
    k = c["kept"]
    if not k.any():
        return 0.0
    err = (emu[k] - c["cdf"][k]).abs().max(-1)[0]
    return float((err / c["bound"][k]).max())


# ---- samples ---------------------------------------------------------------------------------------------------------------------------
def sample_bars(bins, cdf, u, knot_bar):
    """Reference samples of the inverse CDF (oracle._inverse_cdf, float64) with a bar per sample and the mask of compared samples.

    bins, cdf [R,n] float64; u [R,N]; knot_bar [R]: the bar of the ray's CDF knots.  d sample <= bar x (z[above] - z[below]) / den
    (the derivative of the lerp wrt its two knots sums to that) + 4 ulp of 6 (the lerp's own float32 operations).  den is the
    effective denominator (1 where den < 1e-5).  Left out:
      * a sample whose bin's den lies within 2 bars of 1e-5 (the kernel may take the other side of the rule);
      * a sample whose u lies within the bar of a knot at which the inverse CDF jumps: a knot whose bin BELOW falls under the rule (from
        below the sample stays at z[k-1], from above it starts at z[k]) or may do so.  Across every other knot the lerp is continuous,
        and the bar takes the steeper of the two bins, since the kernel may land in either."""
    R, n = cdf.shape
    u = f64(u).expand(R, -1).contiguous()
    ref = O._inverse_cdf(bins, cdf, u)
    bar = knot_bar[:, None]
    den = torch.cat([cdf[:, 1:] - cdf[:, :-1], torch.zeros_like(cdf[:, :1])], -1)       # bin j = [knot j, knot j+1); bin n-1: past the end
    dz = torch.cat([bins[:, 1:] - bins[:, :-1], torch.zeros_like(cdf[:, :1])], -1)
    rule = den < 1e-5
    at_rule = (den - 1e-5).abs() <= 2 * bar
    slope = dz / torch.where(rule, torch.ones_like(den), den)
    jump = torch.cat([torch.zeros_like(rule[:, :1]), (rule | at_rule)[:, :-1]], -1)          # jump[k]: bin k-1 is (or may be) a rule bin
    b = (torch.searchsorted(cdf, u, right=True) - 1).clamp(0, n - 1)
    up = (b + 1).clamp(max=n - 1)
    near_lo = (u - cdf.gather(1, b)).abs() <= bar
    near_hi = ((u - cdf.gather(1, up)).abs() <= bar) & (b < n - 1)
    out = at_rule.gather(1, b) | (near_lo & jump.gather(1, b)) | (near_hi & jump.gather(1, up))
    steep = slope.gather(1, b)
    steep = torch.where(near_lo, torch.maximum(steep, slope.gather(1, (b - 1).clamp(min=0))), steep)
    steep = torch.where(near_hi, torch.maximum(steep, slope.gather(1, up)), steep)
    return ref, bar * steep + 4 * ULP6, ~out


def u_shared(N):
    return torch.linspace(0.0, 1.0, N)


def u_per_ray(R, N, seed=0):
    return torch.rand(R, N, generator=gen(77 + 13 * N + seed))


# ---- merge, finish, picks, init: plain torch -------------------------------------------------------------------------------------------
def merge_reference(z, samples):
    """Sorted union of z [R,n] (sorted) and samples [R,N] (sorted) by ranks, old first on ties -> merged [R,n+N], order (index into
    cat[z, samples])."""
    R, n = z.shape
    N = samples.shape[1]
    pos_old = torch.arange(n)[None] + (samples[:, None, :] < z[:, :, None]).sum(-1)
    pos_new = torch.arange(N)[None] + (z[:, None, :] <= samples[:, :, None]).sum(-1)
    pos = torch.cat([pos_old, pos_new], -1)
    cat = torch.cat([z, samples], -1)
    merged = torch.empty_like(cat).scatter_(1, pos, cat)
    order = torch.empty_like(pos).scatter_(1, pos, torch.arange(n + N)[None].expand(R, -1).contiguous())
    return merged, order


def rank_sort(rows):
    """Every element to its rank: #(smaller) + #(equal and earlier) -> sorted rows."""
    M = rows.shape[1]
    x, y = rows[:, :, None], rows[:, None, :]
    earlier = torch.arange(M)[None, :] < torch.arange(M)[:, None]
    rank = ((y < x) | ((y == x) & earlier[None])).sum(-1)
    return torch.empty_like(rows).scatter_(1, rank, rows)


def finish_reference(samples, z, pick, near, far):
    """ray_sampler.py:263-273: sort of [samples | near | far | z[:, pick]]."""
    R = samples.shape[0]
    cols = [samples, torch.full((R, 1), near, dtype=samples.dtype), torch.full((R, 1), far, dtype=samples.dtype)]
    if pick is not None and pick.numel():
        cols.append(z[:, pick.long()])
    return rank_sort(torch.cat(cols, -1))


def picks_reference(keys, n, n_extra):
    """The n_extra smallest of the first n keys in key order, equal keys: the lower index first."""
    return torch.argsort(keys[:n], stable=True)[:n_extra]


def eval_pick(n, n_extra):
    return torch.linspace(0, n - 1, n_extra).long()


def keys_with_ties(n_total, seed=0):
    """Uniforms in [0.01, 1) with groups of equal keys BELOW every other key (distinct values under 1e-3), so that every group a grid
    contains ranks among its first 16 picks and the lower-index-first rule decides their order: a pair and a run of four inside the
    first 256 keys, a group that straddles index 256 (250, 256, 260), a pair that straddles index 512 (500, 520), a group spread over
    three parts of 256 keys (7, 300, 600), and the first with the last key."""
    k = torch.rand(n_total, generator=gen(900 + seed + n_total)) * 0.99 + 0.01
    k[3] = k[5] = 1e-4
    if n_total > 30:
        k[17:21] = 2e-4
    for group, value in (((250, 256, 260), 3e-4), ((500, 520), 4e-4), ((7, 300, 600), 5e-4)):
        members = [i for i in group if i < n_total]
        if len(members) > 1:
            k[torch.tensor(members)] = value
    k[0] = k[n_total - 1] = 6e-4
    return k


def tied_pair_across_parts(keys, picks):
    """Whether the picks hold two equal keys whose indices lie in different 256-key parts."""
    picks = picks.tolist()
    return any(keys[i] == keys[j] and i // 256 != j // 256 for a, i in enumerate(picks) for j in picks[a + 1:])


def init_reference(z, beta_param, beta_min, eps=EPS):
    """-> beta0 float32 (|beta| + beta_min: one float32 addition, exact to compare), per-ray beta float64."""
    beta0 = torch.tensor(beta_param, dtype=F32).abs() + torch.tensor(beta_min, dtype=F32)
    z64 = f64(z)
    return beta0, torch.sqrt(beta_c(eps) * ((z64[:, 1:] - z64[:, :-1]) ** 2).sum(-1))


def x_fm_reference(origins, dirs, z, ldp):
    """o + (z d), product rounded then the sum, feature-major [3, ldp] with zero padding (float32 chain, bit for bit)."""
    R, n = z.shape
    x = origins[:, None, :] + z[:, :, None] * dirs[:, None, :]
    out = torch.zeros(3, ldp)
    out[:, :R * n] = x.reshape(R * n, 3).t()
    return out


PDF_SHAPES = [(2, 1), (3, 64), (64, 65), (65, 64), (66, 1), (129, 65), (1024, 64)]
PDF_CASES = [(nb, N, zeros) for nb, N in PDF_SHAPES for zeros in (False, True) if nb > 2 or not zeros]      # (one bin: none to empty)


# ---- sample_pdf --------------------------------------------------------------------------------------------------------------------------
def pdf_inputs(nb, R=16, seed=0, zeros=False):
    """bins [R,nb] sorted in [0, 6], weights [R,nb-1]: dense in [0.05, 1.05], or -- zeros -- with stretches of exact zeros and a row sum
    of at least 1.5 (the empty bins then sit a third below the `den < 1e-5` rule: 1e-5 / (1.5 + nb 1e-5) <= 0.667e-5)."""
    g = gen(5000 + 17 * nb + seed + (1 if zeros else 0))
    bins = (torch.rand(R, nb, generator=g) * 6).sort(-1)[0]
    w = torch.rand(R, nb - 1, generator=g) + 0.05
    if zeros:
        m = nb - 1
        keep = torch.zeros(R, m, dtype=torch.bool)
        for r in range(R):
            start = int(torch.randint(0, m, (1,), generator=g))
            keep[r, start:start + max(1, m // 3)] = True
            if m >= 4:
                keep[r, (start * 7 + 3) % m] = True
        w = w * keep
        w = w * (2.0 / w.sum(-1, keepdim=True))                 # row sum 2 (>= 1.5 with float32 rounding to spare)
    return bins, w


def pdf_reference(bins, w, u):
    """oracle.sample_pdf in float64 -> samples, bars, compared mask, and the margin of the empty bins from the rule."""
    b64, w64 = f64(bins), f64(w)
    p = w64 + 1e-5
    cdf = _cdf_of(p)
    ref, bar, cmp_ = sample_bars(b64, cdf, u, torch.full((bins.shape[0],), PDF_KNOT_BAR, dtype=F64))
    assert torch.equal(ref, O.sample_pdf(b64, w64, f64(u).expand(bins.shape[0], -1)))
    den = cdf[:, 1:] - cdf[:, :-1]
    return ref, bar, cmp_, den


def rule_margin(den):
    """Smallest relative distance of a bin's mass from the 1e-5 rule."""
    return float(((den - 1e-5).abs() / 1e-5).min())


def pdf_emulation(bins, w, u, carry=True):
    """sample_pdf_kernel's arithmetic on the CPU: float32 pdf / sum, float64 scans over 64-bin chunks with a carry, one rounding per
    knot.  carry=False is the defect the sizes past one chunk are there to catch."""
    p = w.to(F32) + 1e-5
    q = p / p.to(F64).sum(-1, keepdim=True).to(F32)
    knots, run = [], torch.zeros(q.shape[0], 1, dtype=F64)
    for c0 in range(0, q.shape[1], 64):
        incl = torch.cumsum(q[:, c0:c0 + 64].to(F64), -1)
        knots.append((run + incl).to(F32))
        if carry:
            run = run + incl[:, -1:]
    cdf = torch.cat([torch.zeros_like(q[:, :1])] + knots, -1)
    return O._inverse_cdf(bins.to(F32), cdf, u.to(F32).expand(q.shape[0], -1).contiguous())
