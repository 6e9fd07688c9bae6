// The zero-level surface of an SDF grid as an indexed triangle mesh (the reference's plots.get_surface_trace, code/utils/plots.py:101-138,
// evaluates the grid in 100 000-point chunks through PyTorch and runs skimage's marching cubes on the host): the grid's query points
// written straight into the SDF kernels' feature-major layout, and marching tetrahedra on the device.  All arithmetic is fp32 / int32
// (node coordinates: float64 rounded once, numpy.linspace's arithmetic); no atomics, every scan has a fixed order, so two runs give the
// same bytes.  Nothing here synchronises with the host: the vertex and face counts are written to device memory and read once by the
// caller between mesh_count / mesh_scan and mesh_verts / mesh_faces.
//
// Definitions (tests/mesh_f64.py restates them in float64):
//   node (i, j, k) of a grid [nx][ny][nz] has linear index (i ny + j) nz + k; a cell is named by its lowest node
//   inside      v < level (NaN is outside)
//   edge        class c = 0..6 of a node joins it to the node at offset (dx, dy, dz) = bits (4, 2, 1) of c + 1 (3 axis edges, 3 face
//               diagonals, the body diagonal); it carries a vertex iff its two nodes differ in `inside` and both values are finite
//   vertex      a + t (b - a), t = (level - va) / (vb - va), a the inside node, b the outside node
//   cell        the six tetrahedra 0 -> e_p -> e_p + e_q -> (1,1,1) around the main diagonal, (p, q, r) the permutations of (x, y, z) in
//               lexicographic order (MESH_TET, each positively oriented); neighbouring cells split every shared face along the same
//               diagonal, so the mesh is closed wherever the surface does not leave the grid; a tetrahedron with a non-finite corner
//               emits nothing
//   order       vertices ascending (node, class); faces ascending (cell, tetrahedron, triangle); normals towards increasing values
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "block_util.hpp"        // block_exscan, block_sum
#include "device_util.hpp"       // rounded

namespace neat {

constexpr int MESH_WG = 256;
constexpr int MESH_TILE = 2048;        // nodes per workgroup: MESH_TILE / MESH_WG sub-chunks of consecutive nodes, one node per thread

// corner codes (bit 4 = +x, 2 = +y, 1 = +z) of the six tetrahedra, det(c1 - c0, c2 - c0, c3 - c0) > 0
__constant__ const unsigned char MESH_TET[6][4] = {{0, 4, 6, 7}, {0, 5, 4, 7}, {0, 6, 2, 7}, {0, 2, 3, 7}, {0, 1, 5, 7}, {0, 3, 1, 7}};
// mask = bit l set iff local corner l is inside.  One inside (or one outside) corner p: the triangle of p's three edges; two and two:
// the quad p1q1, p1q2, p2q2, p2q1 split along its first diagonal.  Entries are local edges (a << 2) | b, a < b.
__constant__ const unsigned char MESH_NTRI[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
__constant__ const unsigned char MESH_TRI[16][6] = {
    {0, 0, 0, 0, 0, 0},  {1, 2, 3, 0, 0, 0},  {1, 7, 6, 0, 0, 0},  {2, 3, 7, 2, 7, 6},  {2, 6, 11, 0, 0, 0}, {1, 11, 3, 1, 6, 11},
    {1, 7, 11, 1, 11, 2}, {3, 7, 11, 0, 0, 0}, {3, 11, 7, 0, 0, 0}, {1, 2, 11, 1, 11, 7}, {1, 11, 6, 1, 3, 11}, {2, 11, 6, 0, 0, 0},
    {2, 6, 7, 2, 7, 3},  {1, 6, 7, 0, 0, 0},  {1, 3, 2, 0, 0, 0},  {0, 0, 0, 0, 0, 0}};

struct MeshAxes {
  double b0[3], step[3], b1[3];     // node i of axis a: float(b0 + i step), the last node exactly b1 (numpy.linspace)
  int n[3];
};

__device__ __forceinline__ float mesh_coord(const MeshAxes& g, int a, int i) {
  // the product and the sum are rounded separately, as numpy.linspace does (__dmul_rn / __dadd_rn are plain operators and were contracted
  // into one v_fma_f64, which parts from the rule where b0 + i step cancels to a node next to zero)
  return i == g.n[a] - 1 ? (float)g.b1[a] : (float)rounded(rounded((double)i * g.step[a]) + g.b0[a]);
}

// ---- (a) the query points of `count` consecutive nodes from node `first` into x_fm [3][ldp]; the layout's padding columns are zeroed
__global__ __launch_bounds__(256) void grid_points_kernel(float* __restrict__ x_fm, int ldp, long long first, int count, MeshAxes g) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= ldp) return;
  float x = 0.f, y = 0.f, z = 0.f;
  if (p < count) {
    const long long node = first + p;
    const long long ij = node / g.n[2];
    x = mesh_coord(g, 0, (int)(ij / g.n[1]));
    y = mesh_coord(g, 1, (int)(ij % g.n[1]));
    z = mesh_coord(g, 2, (int)(node % g.n[2]));
  }
  x_fm[p] = x;
  x_fm[(size_t)ldp + p] = y;
  x_fm[2 * (size_t)ldp + p] = z;
}

// ---- (b) marching tetrahedra
struct MeshArgs {
  const float* grid; int nx, ny, nz; int nodes; float level;
  unsigned char* emask;     // [nodes] bit c: edge class c of the node carries a vertex
  int* vbase;               // [nodes] index of the node's first vertex
  int* tile_v; int* tile_f; // [tiles] counts, then (mesh_scan_kernel) exclusive offsets
  int* counts;              // nv, nf (or -1, -1: more than int32 holds)
  MeshAxes ax;
  float* verts; int nv;
  int* faces; int nf;
};

// the node's own value and its seven upper neighbours as `inside` / `finite` bits per corner code; a corner outside the grid is non-finite
__device__ __forceinline__ void mesh_corner_bits(const MeshArgs& a, int node, bool live, unsigned& in, unsigned& fin) {
  in = 0; fin = 0;
  if (!live) return;
  const int k = node % a.nz, ij = node / a.nz, j = ij % a.ny, i = ij / a.ny;
  const bool ux = i + 1 < a.nx, uy = j + 1 < a.ny, uz = k + 1 < a.nz;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const bool ok = (!(c & 4) || ux) && (!(c & 2) || uy) && (!(c & 1) || uz);
    if (!ok) continue;
    const float v = a.grid[(size_t)node + (size_t)((c >> 2) & 1) * a.ny * a.nz + (size_t)((c >> 1) & 1) * a.nz + (c & 1)];
    in |= (v < a.level ? 1u : 0u) << c;
    fin |= (isfinite(v) ? 1u : 0u) << c;
  }
}

__device__ __forceinline__ unsigned mesh_edge_mask(unsigned in, unsigned fin) {
  return ((in >> 1) ^ ((in & 1) ? 0x7fu : 0u)) & (fin >> 1) & ((fin & 1) ? 0x7fu : 0u);
}

__device__ __forceinline__ unsigned mesh_tet_case(unsigned in, unsigned fin, int t) {      // 0 for a tetrahedron that emits nothing
  unsigned m = 0, ok = 1;
#pragma unroll
  for (int l = 0; l < 4; ++l) { const unsigned c = MESH_TET[t][l]; m |= ((in >> c) & 1u) << l; ok &= (fin >> c) & 1u; }
  return ok ? m : 0u;
}

__device__ __forceinline__ int mesh_cell_faces(unsigned in, unsigned fin) {
  int n = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) n += MESH_NTRI[mesh_tet_case(in, fin, t)];
  return n;
}

// pass 1: the edge bits of every node, and per tile the number of vertices and faces
__global__ __launch_bounds__(MESH_WG) void mesh_count_kernel(MeshArgs a) {
  __shared__ int s_wave[MESH_WG / 64];
  int nv = 0, nf = 0;
  for (int s0 = 0; s0 < MESH_TILE; s0 += MESH_WG) {
    const long long nl = (long long)blockIdx.x * MESH_TILE + s0 + threadIdx.x;
    const bool live = nl < a.nodes;
    unsigned in, fin;
    mesh_corner_bits(a, (int)nl, live, in, fin);
    const unsigned em = mesh_edge_mask(in, fin);
    if (live) a.emask[nl] = (unsigned char)em;
    nv += __popc(em);
    nf += mesh_cell_faces(in, fin);
  }
  nv = block_sum<MESH_WG>(nv, s_wave);
  nf = block_sum<MESH_WG>(nf, s_wave);
  if (threadIdx.x == 0) { a.tile_v[blockIdx.x] = nv; a.tile_f[blockIdx.x] = nf; }
}

// pass 2, one workgroup of 1024: the tile counts become exclusive offsets, in tile order; totals in 64 bits
__global__ __launch_bounds__(1024) void mesh_scan_kernel(int* __restrict__ tile_v, int* __restrict__ tile_f, int tiles, int* __restrict__ counts) {
  __shared__ int s_wave[16];
  long long cv = 0, cf = 0;
  for (int t0 = 0; t0 < tiles; t0 += 1024) {      // both counts in one walk (block_carry_scan twice would wait for twice the loads)
    const int t = t0 + threadIdx.x;
    const int v = t < tiles ? tile_v[t] : 0, f = t < tiles ? tile_f[t] : 0;
    int tv, tf;
    const int ev = block_exscan(v, s_wave, &tv), ef = block_exscan(f, s_wave, &tf);
    if (t < tiles) {      // past int32 the offsets are never used: the caller sees counts = -1 and does not emit
      tile_v[t] = (int)min(cv + ev, (long long)INT_MAX);
      tile_f[t] = (int)min(cf + ef, (long long)INT_MAX);
    }
    cv += tv; cf += tf;
  }
  if (threadIdx.x == 0) {
    const bool ok = cv <= INT_MAX && cf <= INT_MAX;
    counts[0] = ok ? (int)cv : -1;
    counts[1] = ok ? (int)cf : -1;
  }
}

// pass 3: every node's first vertex index, and the vertices
__global__ __launch_bounds__(MESH_WG) void mesh_verts_kernel(MeshArgs a) {
  __shared__ int s_wave[MESH_WG / 64];
  int carry = a.tile_v[blockIdx.x];
  for (int s0 = 0; s0 < MESH_TILE; s0 += MESH_WG) {
    const long long nl = (long long)blockIdx.x * MESH_TILE + s0 + threadIdx.x;
    const bool live = nl < a.nodes;
    const int node = (int)nl;
    const unsigned em = live ? a.emask[nl] : 0u;
    int tot;
    const int base = carry + block_exscan(__popc(em), s_wave, &tot);
    carry += tot;
    if (!live) continue;
    a.vbase[node] = base;
    if (!em) continue;
    const int k = node % a.nz, ij = node / a.nz, j = ij % a.ny, i = ij / a.ny;
    const float va = a.grid[node];
    const float ax = mesh_coord(a.ax, 0, i), ay = mesh_coord(a.ax, 1, j), az = mesh_coord(a.ax, 2, k);
    int r = 0;
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      if (!((em >> c) & 1u)) continue;
      const int dx = ((c + 1) >> 2) & 1, dy = ((c + 1) >> 1) & 1, dz = (c + 1) & 1;
      const float vb = a.grid[(size_t)node + (size_t)dx * a.ny * a.nz + (size_t)dy * a.nz + dz];
      const float bx = dx ? mesh_coord(a.ax, 0, i + 1) : ax, by = dy ? mesh_coord(a.ax, 1, j + 1) : ay, bz = dz ? mesh_coord(a.ax, 2, k + 1) : az;
      const bool a_in = va < a.level;                       // from the inside node towards the outside node
      const float vs = a_in ? va : vb, ve = a_in ? vb : va;
      const float t = __fdiv_rn(__fsub_rn(a.level, vs), __fsub_rn(ve, vs));
      const float sx = a_in ? ax : bx, sy = a_in ? ay : by, sz = a_in ? az : bz;
      const float ex = a_in ? bx : ax, ey = a_in ? by : ay, ez = a_in ? bz : az;
      const int o = base + r++;
      if (o < a.nv) {
        float* q = a.verts + 3 * (size_t)o;
        q[0] = __fadd_rn(sx, __fmul_rn(t, __fsub_rn(ex, sx)));
        q[1] = __fadd_rn(sy, __fmul_rn(t, __fsub_rn(ey, sy)));
        q[2] = __fadd_rn(sz, __fmul_rn(t, __fsub_rn(ez, sz)));
      }
    }
  }
}

// pass 4: the faces, through emask / vbase of the edge's owner node
__global__ __launch_bounds__(MESH_WG) void mesh_faces_kernel(MeshArgs a) {
  __shared__ int s_wave[MESH_WG / 64];
  int carry = a.tile_f[blockIdx.x];
  const size_t sx = (size_t)a.ny * a.nz, sy = (size_t)a.nz;
  for (int s0 = 0; s0 < MESH_TILE; s0 += MESH_WG) {
    const long long nl = (long long)blockIdx.x * MESH_TILE + s0 + threadIdx.x;
    const bool live = nl < a.nodes;
    unsigned in, fin;
    mesh_corner_bits(a, (int)nl, live, in, fin);
    const int cnt = mesh_cell_faces(in, fin);
    int tot;
    int f = carry + block_exscan(cnt, s_wave, &tot);
    carry += tot;
    if (cnt == 0) continue;
    for (int t = 0; t < 6; ++t) {
      const unsigned m = mesh_tet_case(in, fin, t);
      const int ntri = MESH_NTRI[m];
      for (int s = 0; s < ntri; ++s, ++f) {
        int idx[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          const unsigned e = MESH_TRI[m][3 * s + v];
          const unsigned ca = MESH_TET[t][e >> 2], cb = MESH_TET[t][e & 3];
          const unsigned lo = min(ca, cb), hi = max(ca, cb);              // the edge's owner is its lower node; its class the offset - 1
          const size_t owner = (size_t)nl + ((lo >> 2) & 1) * sx + ((lo >> 1) & 1) * sy + (lo & 1);
          const unsigned cls = (lo ^ hi) - 1u;
          idx[v] = a.vbase[owner] + __popc((unsigned)a.emask[owner] & ((1u << cls) - 1u));
        }
        if (f < a.nf) {
          int* q = a.faces + 3 * (size_t)f;
          q[0] = idx[0]; q[1] = idx[1]; q[2] = idx[2];
        }
      }
    }
  }
}

// ---- (c) unit normals: rows of g [n,3] scaled to length one in place (a zero row stays zero)
__global__ __launch_bounds__(256) void mesh_normalize_kernel(float* __restrict__ g, int n) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  float* q = g + 3 * (size_t)p;
  const float x = q[0], y = q[1], z = q[2];
  const float inv = 1.0f / fmaxf(sqrtf((x * x + y * y) + z * z), 1e-12f);
  q[0] = x * inv; q[1] = y * inv; q[2] = z * inv;
}

}  // namespace neat
