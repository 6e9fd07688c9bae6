// Wireframe parsing of a trained model (code/neat-final-parsing.py: initial_recon :159-302, get_wireframe_from_lines_and_junctions
// :134-157, visibility_checking :305-336) as device launches: the per-view line matching, the per-label grouping, the junction
// vote, the junction graph and the visibility count.  All arithmetic is fp32; there are no float atomics (no atomics at all), every
// reduction has a fixed shape, so every result is bit-identical from run to run.  Nothing here synchronises with the host: counts
// that size an output (labels present, lines kept, junctions, edges) are written to device memory and read once by the caller.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "block_util.hpp"           // block_exscan, block_compact
#include "kernels_junction.hpp"     // project_point (VolSDFNetwork.project2D's arithmetic)

namespace neat {

constexpr int PARSE_WG = 256;
constexpr int PARSE_GT_CHUNK = 1024;     // ground-truth lines staged in LDS per chunk (16 KB of float4)
constexpr int PARSE_TILE = 4096;         // rows per tile of the stable counting sort (16 sub-chunks of PARSE_WG rows)

__device__ __forceinline__ float parse_d4(float a0, float a1, float a2, float a3, const float4& g) {
  const float d0 = a0 - g.x, d1 = a1 - g.y, d2 = a2 - g.z, d3 = a3 - g.w;
  return ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
}

// ---- line match (:226-236): one thread per predicted line, both orientations (row i = the line, row n + i = its reverse
// (x2, y2, x1, y1)); the ground-truth lines go through LDS in chunks and every lane reads the same entry (a broadcast).
// label[r] = argmin_j |row_r - gt_j|^2 (lowest j on ties) if that minimum is < thr, else -1; mindis[r] = the minimum (+inf for m = 0,
// NaN if any distance of the row is NaN: such a row never matches, as `NaN < thr` is false for the reference).
__global__ __launch_bounds__(PARSE_WG) void parse_match_kernel(const float* __restrict__ lines2d, int n, const float* __restrict__ gt,
                                                               int m, int gt_stride, float thr, int* __restrict__ label,
                                                               float* __restrict__ mindis) {
  __shared__ float4 s_gt[PARSE_GT_CHUNK];
  const int i = blockIdx.x * PARSE_WG + threadIdx.x;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (i < n) { a0 = lines2d[4 * (size_t)i]; a1 = lines2d[4 * (size_t)i + 1]; a2 = lines2d[4 * (size_t)i + 2]; a3 = lines2d[4 * (size_t)i + 3]; }
  float bf = INFINITY, br = INFINITY;
  int jf = -1, jr = -1;
  bool nf = false, nr = false;
  for (int c0 = 0; c0 < m; c0 += PARSE_GT_CHUNK) {
    const int cn = min(PARSE_GT_CHUNK, m - c0);
    __syncthreads();
    for (int k = threadIdx.x; k < cn; k += PARSE_WG) {
      const float* g = gt + (size_t)(c0 + k) * gt_stride;
      s_gt[k] = make_float4(g[0], g[1], g[2], g[3]);
    }
    __syncthreads();
    if (i < n) {
      for (int k = 0; k < cn; ++k) {
        const float4 g = s_gt[k];
        const float df = parse_d4(a0, a1, a2, a3, g), dr = parse_d4(a2, a3, a0, a1, g);
        if (df != df) nf = true; else if (df < bf) { bf = df; jf = c0 + k; }
        if (dr != dr) nr = true; else if (dr < br) { br = dr; jr = c0 + k; }
      }
    }
  }
  if (i >= n) return;
  mindis[i] = nf ? NAN : bf;
  mindis[(size_t)n + i] = nr ? NAN : br;
  label[i] = (!nf && bf < thr) ? jf : -1;
  label[(size_t)n + i] = (!nr && br < thr) ? jr : -1;
}

// ---- group (:237-257): a stable counting sort of the matched rows by label, then one workgroup per label.
// Pass 0 (count) and pass 1 (scatter) walk a tile of PARSE_TILE rows in sub-chunks of PARSE_WG rows; within a sub-chunk a row's rank
// among the earlier rows with its label comes from an LDS scan (no atomics), and the last row of each label advances that label's
// running counter of the tile (`run`, [nt][m]; one writer per label and sub-chunk, ordered by the barriers).
__global__ __launch_bounds__(PARSE_WG) void parse_group_tile_kernel(const int* __restrict__ label, int rows, int m, int* __restrict__ run,
                                                                    int* __restrict__ order, int scatter) {
  __shared__ int s_lab[PARSE_WG];
  const int t = blockIdx.x, tid = threadIdx.x;
  int* trun = run + (size_t)t * m;
  for (int s0 = 0; s0 < PARSE_TILE; s0 += PARSE_WG) {
    const int r = t * PARSE_TILE + s0 + tid;
    const int l = r < rows ? label[r] : -1;
    s_lab[tid] = l;
    __syncthreads();
    int before = 0, total = 0, base = 0;
    if (l >= 0) {
      for (int j = 0; j < PARSE_WG; ++j) {
        const int e = s_lab[j] == l;
        before += (j < tid) & e;
        total += e;
      }
      base = trun[l];
    }
    __syncthreads();                                           // every row has read its label's counter before one of them advances it
    if (l >= 0) {
      if (scatter) order[base + before] = r;
      if (before == total - 1) trun[l] = base + total;        // the label's last row in this sub-chunk
    }
    __syncthreads();
  }
}

// one workgroup of 1024: per label, the per-tile counts become absolute start positions of each tile's rows (exclusive prefix over
// tiles + the label's start), cnt[l] = rows of label l, slot[l] = rank of l among the labels present (ascending) or -1; *count = L
__global__ __launch_bounds__(1024) void parse_group_scan_kernel(int* __restrict__ run, int nt, int m, int* __restrict__ cnt,
                                                                int* __restrict__ start, int* __restrict__ slot, int* __restrict__ count) {
  __shared__ int s_wave[16];
  int carry = 0, carry_present = 0;
  for (int l0 = 0; l0 < m; l0 += 1024) {      // both scans in one walk over the labels (as mesh_scan_kernel)
    const int l = l0 + threadIdx.x;
    int c = 0;
    if (l < m) {
      for (int t = 0; t < nt; ++t) { const int h = run[(size_t)t * m + l]; run[(size_t)t * m + l] = c; c += h; }
      cnt[l] = c;
    }
    int tot, totp;
    const int st = block_exscan(c, s_wave, &tot);
    const int sp = block_exscan(c > 0 ? 1 : 0, s_wave, &totp);
    if (l < m) {
      start[l] = carry + st;
      slot[l] = c > 0 ? carry_present + sp : -1;
      for (int t = 0; t < nt; ++t) run[(size_t)t * m + l] += carry + st;
    }
    carry += tot;
    carry_present += totp;
  }
  if (threadIdx.x == 0) *count = carry_present;
}

// fixed-shape sum of PARSE_WG values (same tree every run)
template <int C>
__device__ __forceinline__ void parse_block_sum(float (&v)[C], float (*s)[PARSE_WG]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int c = 0; c < C; ++c) s[c][tid] = v[c];
  __syncthreads();
  for (int h = PARSE_WG / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int c = 0; c < C; ++c) s[c][tid] += s[c][tid + h];
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = s[c][0];
  __syncthreads();
}

// one workgroup per label l present: v = mean of its rows' lines3d (rows >= n are the reversed lines), score = mean over the same rows of
// |(p - v0) x (p - v1)| / max(|v1 - v0|, 1e-6), p = the row's l3d.  Written at slot[l]: the labels in ascending order.
__global__ __launch_bounds__(PARSE_WG) void parse_group_reduce_kernel(const int* __restrict__ order, const int* __restrict__ cnt,
                                                                      const int* __restrict__ start, const int* __restrict__ slot,
                                                                      const float* __restrict__ lines3d, const float* __restrict__ l3d, int n,
                                                                      float* __restrict__ lines, float* __restrict__ scores) {
  __shared__ float s_red[6][PARSE_WG];
  const int l = blockIdx.x, tid = threadIdx.x;
  const int c = cnt[l];
  if (c == 0) return;
  const int* seg = order + start[l];
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k = tid; k < c; k += PARSE_WG) {
    const int r = seg[k];
    const bool rev = r >= n;
    const float* L = lines3d + 6 * (size_t)(rev ? r - n : r);
#pragma unroll
    for (int q = 0; q < 3; ++q) { acc[q] += L[rev ? 3 + q : q]; acc[3 + q] += L[rev ? q : 3 + q]; }
  }
  parse_block_sum<6>(acc, s_red);
  float v[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) v[q] = acc[q] / (float)c;
  const float e0 = v[3] - v[0], e1 = v[4] - v[1], e2 = v[5] - v[2];
  const float den = fmaxf(sqrtf(e0 * e0 + e1 * e1 + e2 * e2), 1e-6f);
  float sc[1] = {0.f};
  for (int k = tid; k < c; k += PARSE_WG) {
    const int r = seg[k];
    const float* p = l3d + 3 * (size_t)(r >= n ? r - n : r);
    const float a0 = p[0] - v[0], a1 = p[1] - v[1], a2 = p[2] - v[2];
    const float b0 = p[0] - v[3], b1 = p[1] - v[4], b2 = p[2] - v[5];
    const float x = a1 * b2 - a2 * b1, y = a2 * b0 - a0 * b2, z = a0 * b1 - a1 * b0;
    sc[0] += sqrtf(x * x + y * y + z * z) / den;
  }
  parse_block_sum<1>(sc, s_red);
  if (tid == 0) {
    const int o = slot[l];
#pragma unroll
    for (int q = 0; q < 6; ++q) lines[6 * (size_t)o + q] = v[q];
    scores[o] = sc[0] / (float)c;
  }
}

// ---- vote (:259-272): cost [J, nc] = |junction_j - endpoint_c| by direct differences (endpoint c = lines.reshape(-1, 3)[c]); columns
// c >= 2 L (L on the device) are masked out of the assignment.
__global__ void parse_vote_cost_kernel(const float* __restrict__ junc, int J, const float* __restrict__ lines, const int* __restrict__ count,
                                       int nc, float* __restrict__ cost, unsigned char* __restrict__ col_mask) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)J * nc) return;
  const int j = (int)(e / nc), c = (int)(e % nc);
  const int ncol = 2 * *count;
  float d = 0.f;
  if (c < ncol) {
    const float d0 = junc[3 * j] - lines[3 * c], d1 = junc[3 * j + 1] - lines[3 * c + 1], d2 = junc[3 * j + 2] - lines[3 * c + 2];
    d = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
  }
  cost[e] = d;
  if (j == 0) col_mask[c] = c < ncol ? 1 : 0;
}

// each assigned pair (rows are distinct within a view) with cost < thr gives its junction one vote; the first vote a junction receives
// stamps (view, pair index): the reference's dict insertion order
__global__ void parse_vote_apply_kernel(const long long* __restrict__ rows, const long long* __restrict__ cols, const int* __restrict__ n_match,
                                        int kmax, const float* __restrict__ cost, int nc, float thr, int view, int* __restrict__ votes,
                                        int* __restrict__ first) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= kmax || k >= *n_match) return;
  const long long i = rows[k], c = cols[k];
  if (i < 0 || c < 0) return;
  if (cost[(size_t)i * nc + c] < thr) {
    const int v = votes[i];
    if (v == 0) { first[2 * i] = view; first[2 * i + 1] = k; }
    votes[i] = v + 1;
  }
}

// ---- wireframe (:278-295, :134-157).  Workgroup 0: the lines of every view with score < thr, in view then label order (ordered
// compaction over the V x mcap slots, view v holding counts[v] lines).  Workgroup 1: the junctions with more than one vote, in the order of
// their first vote.  counts_out[0] = N lines, counts_out[1] = K junctions.
__global__ __launch_bounds__(1024) void parse_select_kernel(const float* __restrict__ vlines, const float* __restrict__ vscores,
                                                            const int* __restrict__ vcount, int V, int mcap, float score_thr,
                                                            const float* __restrict__ junc, const int* __restrict__ votes,
                                                            const int* __restrict__ first, int J, float* __restrict__ lines_out,
                                                            float* __restrict__ junc_out, int* __restrict__ idx_ws, int* __restrict__ counts_out) {
  __shared__ int s_wave[16], s_base;
  const int tid = threadIdx.x;
  if (blockIdx.x == 0) {
    const int total = V * mcap;
    const int N = block_compact(total, [&](int s) { return (s % mcap) < vcount[s / mcap] && vscores[s] < score_thr; }, idx_ws, s_wave, &s_base);
    __syncthreads();
    for (int e = tid; e < 6 * N; e += blockDim.x) lines_out[e] = vlines[6 * (size_t)idx_ws[e / 6] + e % 6];
    if (tid == 0) counts_out[0] = N;
  } else {
    int K = 0;
    for (int j = tid; j < J; j += blockDim.x) {
      if (votes[j] <= 1) continue;
      const int fv = first[2 * j], fk = first[2 * j + 1];
      int rank = 0;
      for (int q = 0; q < J; ++q) {
        if (votes[q] <= 1) continue;
        const int qv = first[2 * q], qk = first[2 * q + 1];
        rank += (qv < fv) || (qv == fv && qk < fk);
      }
#pragma unroll
      for (int d = 0; d < 3; ++d) junc_out[3 * rank + d] = junc[3 * j + d];
    }
    for (int j = tid; j < J; j += blockDim.x) K += votes[j] > 1;
    int tot;
    block_exscan(K, s_wave, &tot);
    if (tid == 0) counts_out[1] = tot;
  }
}

// one thread per kept line: the nearest junction of each end point (lowest index on ties); matched if max(d1, d2) < |ep1 - ep2|; the
// symmetric 0/1 graph [K, K] (row stride ldg) gets both entries.  Several lines may mark one cell: every store writes the same byte.
__global__ __launch_bounds__(PARSE_WG) void parse_graph_mark_kernel(const float* __restrict__ lines, const float* __restrict__ junc,
                                                                    const int* __restrict__ counts, int ncap, int ldg,
                                                                    unsigned char* __restrict__ graph) {
  __shared__ float s_j[3 * PARSE_GT_CHUNK];
  const int N = counts[0], K = counts[1];
  const int i = blockIdx.x * PARSE_WG + threadIdx.x;
  float p[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (i < N && i < ncap) {
#pragma unroll
    for (int q = 0; q < 6; ++q) p[q] = lines[6 * (size_t)i + q];
  }
  float b1 = INFINITY, b2 = INFINITY;
  int i1 = -1, i2 = -1;
  for (int c0 = 0; c0 < K; c0 += PARSE_GT_CHUNK) {
    const int cn = min(PARSE_GT_CHUNK, K - c0);
    __syncthreads();
    for (int k = threadIdx.x; k < 3 * cn; k += PARSE_WG) s_j[k] = junc[3 * (size_t)c0 + k];
    __syncthreads();
    for (int k = 0; k < cn; ++k) {
      const float x = s_j[3 * k], y = s_j[3 * k + 1], z = s_j[3 * k + 2];
      const float a0 = p[0] - x, a1 = p[1] - y, a2 = p[2] - z, c0_ = p[3] - x, c1 = p[4] - y, c2 = p[5] - z;
      const float d1 = sqrtf((a0 * a0 + a1 * a1) + a2 * a2), d2 = sqrtf((c0_ * c0_ + c1 * c1) + c2 * c2);
      if (d1 < b1) { b1 = d1; i1 = c0 + k; }
      if (d2 < b2) { b2 = d2; i2 = c0 + k; }
    }
  }
  if (i >= N || i >= ncap || i1 < 0 || i2 < 0) return;
  const float e0 = p[0] - p[3], e1 = p[1] - p[4], e2 = p[2] - p[5];
  if (fmaxf(b1, b2) < sqrtf((e0 * e0 + e1 * e1) + e2 * e2)) {
    graph[(size_t)i1 * ldg + i2] = 1;
    graph[(size_t)i2 * ldg + i1] = 1;
  }
}

// one wave per graph row i < K: rowcnt[i] = #{j >= i : graph[i][j]}
__global__ __launch_bounds__(64) void parse_edge_count_kernel(const unsigned char* __restrict__ graph, const int* __restrict__ counts, int ldg,
                                                              int* __restrict__ rowcnt) {
  const int i = blockIdx.x, K = counts[1], lane = threadIdx.x;
  int c = 0;
  if (i < K) {
    for (int j0 = i; j0 < K; j0 += 64) {
      const int j = j0 + lane;
      c += __popcll(__ballot(j < K && graph[(size_t)i * ldg + j] != 0));
    }
  }
  if (lane == 0) rowcnt[i] = c;
}

// one wave per row: the row's edges (i, j >= i) in column order at its offset (sum of the earlier rows' counts, a fixed-order
// reduction); the edge list is therefore the row-major order of graph.triu().nonzero().  Row 0's wave writes E = counts[2].
__global__ __launch_bounds__(64) void parse_edge_write_kernel(const unsigned char* __restrict__ graph, int* __restrict__ counts, int ldg,
                                                              const int* __restrict__ rowcnt, int nrows, const float* __restrict__ junc,
                                                              int ecap, int* __restrict__ pairs, float* __restrict__ wfi) {
  const int i = blockIdx.x, K = counts[1], lane = threadIdx.x;
  int off = 0;
  for (int q = lane; q < i; q += 64) off += rowcnt[q];
  int tot = 0;
  if (i == 0) for (int q = lane; q < nrows; q += 64) tot += rowcnt[q];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { off += __shfl_xor(off, o); tot += __shfl_xor(tot, o); }
  if (i == 0 && lane == 0) counts[2] = min(tot, ecap);
  if (i >= K) return;
  for (int j0 = i; j0 < K; j0 += 64) {
    const int j = j0 + lane;
    const bool f = j < K && graph[(size_t)i * ldg + j] != 0;
    const unsigned long long bal = __ballot(f);
    const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
    if (f && pos < ecap) {
      pairs[2 * (size_t)pos] = i; pairs[2 * (size_t)pos + 1] = j;
#pragma unroll
      for (int d = 0; d < 3; ++d) { wfi[6 * (size_t)pos + d] = junc[3 * i + d]; wfi[6 * (size_t)pos + 3 + d] = junc[3 * j + d]; }
    }
    off += __popcll(bal);
  }
}

// ---- visibility (:305-336): grid (line tiles, views).  A line is visible in view v if the smallest squared distance of its projection
// (K3_v, w2c_v) to the view's ground-truth lines, in either orientation, is < ckdist.  A view without ground-truth lines sees nothing.
__global__ __launch_bounds__(PARSE_WG) void parse_vis_kernel(const float* __restrict__ lines, const int* __restrict__ n_dev, int ecap,
                                                             const float* __restrict__ gt, int gt_stride, const int* __restrict__ gt_off,
                                                             const float* __restrict__ K3, const float* __restrict__ w2c, float ckdist,
                                                             unsigned char* __restrict__ vis) {
  __shared__ float4 s_gt[PARSE_GT_CHUNK];
  const int v = blockIdx.y;
  const int E = n_dev ? min(*n_dev, ecap) : ecap;
  const int e = blockIdx.x * PARSE_WG + threadIdx.x;
  if ((int)(blockIdx.x * PARSE_WG) >= E) return;       // whole workgroup beyond the lines (uniform exit before any barrier)
  float u[4] = {0.f, 0.f, 0.f, 0.f};
  if (e < E) {
    for (int h = 0; h < 2; ++h) {
      const float x[3] = {lines[6 * (size_t)e + 3 * h], lines[6 * (size_t)e + 3 * h + 1], lines[6 * (size_t)e + 3 * h + 2]};
      float cam[3], w;
      project_point(K3 + 9 * v, w2c + 12 * v, x, cam, w);
      u[2 * h] = cam[0] / w; u[2 * h + 1] = cam[1] / w;
    }
  }
  const int g0 = gt_off[v], m = gt_off[v + 1] - g0;
  float best = INFINITY;
  bool nan = false;
  for (int c0 = 0; c0 < m; c0 += PARSE_GT_CHUNK) {
    const int cn = min(PARSE_GT_CHUNK, m - c0);
    __syncthreads();
    for (int k = threadIdx.x; k < cn; k += PARSE_WG) {
      const float* g = gt + (size_t)(g0 + c0 + k) * gt_stride;
      s_gt[k] = make_float4(g[0], g[1], g[2], g[3]);
    }
    __syncthreads();
    for (int k = 0; k < cn; ++k) {
      const float4 g = s_gt[k];
      const float d1 = parse_d4(u[0], u[1], u[2], u[3], g), d2 = parse_d4(u[2], u[3], u[0], u[1], g);
      if (d1 != d1 || d2 != d2) nan = true;
      else best = fminf(best, fminf(d1, d2));
    }
  }
  if (e < E) vis[(size_t)v * ecap + e] = (m > 0 && !nan && best < ckdist) ? 1 : 0;
}

// one workgroup: vis_count[e] = views that see line e; the lines seen by >= ckview views, in their order -> checked, *n_checked
__global__ __launch_bounds__(1024) void parse_vis_count_kernel(const float* __restrict__ lines, const int* __restrict__ n_dev, int ecap, int V,
                                                               const unsigned char* __restrict__ vis, int ckview, int* __restrict__ vis_count,
                                                               int* __restrict__ idx_ws, float* __restrict__ checked, int* __restrict__ n_checked) {
  __shared__ int s_wave[16], s_base;
  const int E = n_dev ? min(*n_dev, ecap) : ecap;
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    int c = 0;
    for (int v = 0; v < V; ++v) c += vis[(size_t)v * ecap + e];
    vis_count[e] = c;
  }
  __syncthreads();
  const int n = block_compact(E, [&](int e) { return vis_count[e] >= ckview; }, idx_ws, s_wave, &s_base);
  __syncthreads();
  for (int q = threadIdx.x; q < 6 * n; q += blockDim.x) checked[q] = lines[6 * (size_t)idx_ws[q / 6] + q % 6];
  if (threadIdx.x == 0) *n_checked = n;
}

}  // namespace neat
