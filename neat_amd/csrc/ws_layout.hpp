// The workspace of every tool entry point in neat_aux.hip, stated once: a carver, and one layout function per workspace that checks
// the counts, carves a struct of typed pointers and reports the total.  The entry point, its *_ws_bytes query and any offset query
// call that function; with a null base it only measures.  Plain C++ (no HIP): the tile sizes of the kernels come in as arguments, and
// scripts/ws_host_check.cpp runs every layout under the host sanitizers.  Sizes and offsets are part of the ABI (Python allocates
// from the queries; tests/ws_sizes.json pins them).
#pragma once
#include <initializer_list>
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

namespace neat {

inline size_t ws_align(size_t b, size_t a = 256) { return (b + a - 1) & ~(a - 1); }

// A cursor over `base`.  take<T>(count, align) moves the cursor up to a multiple of `align`, returns that place as a T* and advances by
// count elements; end(align) is the size so far, rounded up.  The arithmetic is on integers: over a null base nothing is formed from a
// null pointer, the pointers returned are never dereferenced and ws_offset() of them is the region's offset.
class WsCarver {
 public:
  explicit WsCarver(void* base) : base_((uintptr_t)base) {}
  template <class T>
  T* take(size_t count, size_t align = 256) {
    off_ = ws_align(off_, align);
    T* p = reinterpret_cast<T*>(base_ + off_);
    off_ += count * sizeof(T);
    return p;
  }
  size_t end(size_t align = 256) const { return ws_align(off_, align); }

 private:
  uintptr_t base_;
  size_t off_ = 0;
};
inline size_t ws_offset(const void* base, const void* p) { return (size_t)((uintptr_t)p - (uintptr_t)base); }

// Room for rocprim's radix sort of a list of n keys (with or without values), fixed by n alone so that no workspace size depends on the
// installed rocprim or on a device being present: its temporary keys and values (12 bytes an element at most), its
// histograms and per-block look-back states.  A call asks rocprim and refuses (-2) if it wants more: sort_keys / sort_pairs in neat_aux.hip
inline size_t sort_scratch_bytes(long long n) { return n > 0 ? (size_t)32 * (size_t)n + ((size_t)4 << 20) : 0; }

// ---- lsap: float64 duals, then the int work arrays (LsapArgs in kernels_junction.hpp names them); neither region is padded ------------------
struct LsapWs { double* d; int* i; size_t total; };
inline void lsap_layout(void* ws, int nr, int nc, LsapWs* w) {
  const size_t mx = (size_t)(nr > nc ? nr : nc), mn = (size_t)(nr < nc ? nr : nc);
  WsCarver c(ws);
  w->d = c.take<double>(mn + 2 * mx, 8);
  w->i = c.take<int>((size_t)nr + (size_t)nc + 5 * mx + 2 * mn, 4);
  w->total = c.end(4);
}

struct DbscanWs { int *parent, *has_nb; size_t total; };
inline void dbscan_layout(void* ws, int n, DbscanWs* w) {
  WsCarver c(ws);
  w->parent = c.take<int>((size_t)n, 4);
  w->has_nb = c.take<int>((size_t)n, 4);
  w->total = c.end(4);
}

// ---- wireframe parsing ------------------------------------------------------------------------------------------------------------------------
// group: run [tiles][m] | cnt, start, slot [m] each (one padded block), then order [2 n]; tile = PARSE_TILE rows
struct ParseGroupWs { int tiles; int *run, *cnt, *start, *slot, *order; size_t total; };
inline bool parse_group_layout(void* ws, int n, int m, int tile, ParseGroupWs* w) {
  if (n < 0 || m < 0) return false;
  w->tiles = (2 * n + tile - 1) / tile;
  WsCarver c(ws);
  w->run = c.take<int>((size_t)w->tiles * m);
  w->cnt = c.take<int>((size_t)m, 4);
  w->start = c.take<int>((size_t)m, 4);
  w->slot = c.take<int>((size_t)m, 4);
  w->order = c.take<int>(2 * (size_t)n);
  w->total = c.end();
  return true;
}

// vote: cost [J][nc], nc = 2 mcap | column mask [nc] | rows, cols [k], k = min(J, nc) | n_match | neat_lsap's own workspace of (J, nc)
struct ParseVoteWs { int nc, k; float* cost; unsigned char* cmask; long long *rows, *cols; int* n_match; void* lsap; size_t total; };
inline bool parse_vote_layout(void* ws, int J, int mcap, ParseVoteWs* w) {
  if (J <= 0 || mcap <= 0) return false;
  w->nc = 2 * mcap;
  w->k = J < w->nc ? J : w->nc;
  LsapWs l;
  lsap_layout(nullptr, J, w->nc, &l);
  WsCarver c(ws);
  w->cost = c.take<float>((size_t)J * w->nc);
  w->cmask = c.take<unsigned char>((size_t)w->nc);
  w->rows = c.take<long long>((size_t)w->k);
  w->cols = c.take<long long>((size_t)w->k);
  w->n_match = c.take<int>(1);
  w->lsap = c.take<char>(l.total);
  w->total = c.end();
  return true;
}

struct ParseGraphWs { int *idx, *rowcnt; size_t total; };      // int [V mcap] | int [J]
inline bool parse_graph_layout(void* ws, int V, int mcap, int J, ParseGraphWs* w) {
  if (V < 0 || mcap < 0 || J < 0) return false;
  WsCarver c(ws);
  w->idx = c.take<int>((size_t)V * mcap);
  w->rowcnt = c.take<int>((size_t)J);
  w->total = c.end();
  return true;
}

struct ParseVisWs { unsigned char* vis; int* idx; size_t total; };      // byte [V][ecap] | int [ecap]
inline bool parse_vis_layout(void* ws, int ecap, int V, ParseVisWs* w) {
  if (ecap < 0 || V < 0) return false;
  WsCarver c(ws);
  w->vis = c.take<unsigned char>((size_t)V * ecap);
  w->idx = c.take<int>((size_t)ecap);
  w->total = c.end();
  return true;
}

// ---- surface mesh: edge bits [N] | first vertex index [N] | per-tile vertex and face counts; tile = MESH_TILE nodes ------------------------
struct MeshWs { int nodes, tiles; unsigned char* emask; int *vbase, *tile_v, *tile_f; size_t total; };
inline bool mesh_layout(void* ws, int nx, int ny, int nz, int tile, MeshWs* w) {      // refused: an axis under 2 nodes, or 2^31 nodes and more
  if (nx < 2 || ny < 2 || nz < 2 || (long long)nx * ny > INT_MAX || (long long)nx * ny * nz > INT_MAX) return false;
  w->nodes = nx * ny * nz;
  w->tiles = (int)(((long long)w->nodes + tile - 1) / tile);
  WsCarver c(ws);
  w->emask = c.take<unsigned char>((size_t)w->nodes);
  w->vbase = c.take<int>((size_t)w->nodes);
  w->tile_v = c.take<int>((size_t)w->tiles);
  w->tile_f = c.take<int>((size_t)w->tiles);
  w->total = c.end();
  return true;
}

// ---- the levels of a fixed-shape sum tree (mesh moments, frame sum): the leaf pass turns n inputs into m[0] = ceil(n / leaf) sums of
// `comps` components each, every pass above it `fan` values into one: m[k + 1] = ceil(m[k] / fan) down to m[levels] = 1.  level[k]
// holds the sums of level k < levels as [comps][m[k]]; level[levels] is null: the last value goes to the caller's output
struct SumTreeWs { int levels; long long m[9]; double* level[9]; size_t total; };
inline bool sum_tree_layout(void* ws, long long n, int leaf, int fan, int comps, SumTreeWs* w) {
  if (n < 0) return false;
  WsCarver c(ws);
  int k = 0;
  for (long long m = (n + leaf - 1) / leaf; m > 1; m = (m + fan - 1) / fan, ++k) { w->m[k] = m; w->level[k] = c.take<double>((size_t)comps * (size_t)m, 8); }
  w->levels = k; w->m[k] = 1; w->level[k] = nullptr;
  c.take<double>(1, 8);
  w->total = c.end();
  return true;
}

// the per-workgroup partial results of a two-pass reduction (affine bounds: 6 doubles a block; frame range: 2 floats a block) -> the size
template <class T>
inline size_t partials_layout(void* ws, int blocks, int per_block, T** p) {
  WsCarver c(ws);
  *p = c.take<T>((size_t)blocks * per_block, sizeof(T));
  return c.end(sizeof(T));
}

// ---- evaluation: the grid's histogram [buckets] | bucket of each point [max(n, 1)];  the triangle sampler's counts and offsets [nf + 1] each
struct EvalGridWs { int *cnt, *bucket_of; size_t total; };
inline bool eval_grid_layout(void* ws, int n, int buckets, EvalGridWs* w) {
  if (n < 0 || buckets < 1) return false;
  WsCarver c(ws);
  w->cnt = c.take<int>((size_t)buckets);
  w->bucket_of = c.take<int>((size_t)(n > 1 ? n : 1));
  w->total = c.end();
  return true;
}
struct EvalTriWs { int *counts, *offs; size_t total; };
inline bool eval_tri_layout(void* ws, int nf, EvalTriWs* w) {
  if (nf < 0) return false;
  WsCarver c(ws);
  w->counts = c.take<int>((size_t)nf + 1);
  w->offs = c.take<int>((size_t)nf + 1);
  w->total = c.end();
  return true;
}

// ---- pictures: three planes over F H W pixels (depth keys, line and point coverage), then one 256-byte line with the status word and,
// at +8, the counter of the queue of large triangles, then the queue
struct ShowWs {
  long long pixels;
  unsigned long long* key; unsigned *cov, *covp; int* status; unsigned long long* queued; long long* queue;
  size_t total;
};
inline bool show_layout(void* ws, int F, int H, int W, int queue_cap, ShowWs* s) {
  if (F < 1 || H < 1 || W < 1 || H > 32768 || W > 32768 || (long long)F * H * W > (1ll << 40)) return false;
  s->pixels = (long long)F * H * W;
  WsCarver c(ws);
  s->key = c.take<unsigned long long>((size_t)s->pixels);
  s->cov = c.take<unsigned>((size_t)s->pixels);
  s->covp = c.take<unsigned>((size_t)s->pixels);
  s->status = c.take<int>(1);
  s->queued = c.take<unsigned long long>(1, 8);
  s->queue = c.take<long long>((size_t)queue_cap);
  s->total = c.end(8);
  return true;
}

// ---- sphere tracing: the per-ray state (kernels_trace.hpp reads and writes it through this struct), wg = TRACE_WG rays per workgroup --------
constexpr int TRACE_MAX_RAYS = 1 << 24;      // trace_scan_kernel is one workgroup of 1024 over ceil(R / 256) counts: 64 rounds at most
struct TraceWs {
  float *t;                 // [R] the point of the pending query; for a finished HIT / INSIDE ray its depth
  float *ta, *fa;           // [R] march: the previous point and value; refine: the bracket's end with f >= 0
  float *tb, *fb;           // [R] refine: the bracket's end with f < 0
  float *t1;                // [R] end of the clipped chord
  int *steps, *march, *refine;      // [R] queries made, advances made, refinement rounds made
  unsigned char *phase;     // [R]
  unsigned char *side;      // [R] refine: the end the last query replaced (1 = a, 2 = b, 0 = none yet)
  unsigned char *flag;      // [R] by list position: the entry stays active
  int *ids[2];              // [R] each: the active lists, ping-pong
  int *tile;                // [ceil(R / wg)] active entries per workgroup, then their exclusive offsets
};
inline size_t trace_layout(void* ws, int R, int wg, TraceWs* w) {      // -> the size; 0: refused
  if (R < 1 || R > TRACE_MAX_RAYS) return 0;
  WsCarver c(ws);
  for (float** f : {&w->t, &w->ta, &w->fa, &w->tb, &w->fb, &w->t1}) *f = c.take<float>((size_t)R);
  for (int** i : {&w->steps, &w->march, &w->refine, &w->ids[0], &w->ids[1]}) *i = c.take<int>((size_t)R);
  for (unsigned char** b : {&w->phase, &w->side, &w->flag}) *b = c.take<unsigned char>((size_t)R);
  w->tile = c.take<int>((size_t)((R + wg - 1) / wg));
  return c.end();
}

// ---- fuse / refine / snap of a line soup --------------------------------------------------------------------------------------------------------
constexpr int POST_MAX_GRID = 1024;       // snap: cell keys (ix G + iy) G + iz stay below 2^30
constexpr int POST_MAX_VIEWS = 65535;     // fuse: the views are the y dimension of one launch

// every count that a launch turns into a grid or an int index: lines, views, detections
inline bool post_counts_ok(long long n, long long V, long long mtot) {
  return n >= 0 && V >= 0 && mtot >= 0 && n <= 0x7fffffffLL / 6 && V <= POST_MAX_VIEWS && mtot <= 0x7fffffffLL / 8 &&
         (V == 0 || n <= 0x7fffffffLL / V);
}
inline bool post_grid_ok(long long G) { return G >= 2 && G <= POST_MAX_GRID; }

struct PostFuseWs { int* label; unsigned char* present; int *rank, *idx; size_t total; };        // int [V n] | byte [mtot] | int [mtot] | int [n]
inline bool post_fuse_layout(void* ws, long long n, long long V, long long mtot, PostFuseWs* w) {
  if (!post_counts_ok(n, V, mtot)) return false;
  WsCarver c(ws);
  w->label = c.take<int>((size_t)n * (size_t)V);
  w->present = c.take<unsigned char>((size_t)mtot);
  w->rank = c.take<int>((size_t)mtot);
  w->idx = c.take<int>((size_t)n);
  w->total = c.end();
  return true;
}

// int [2 n] | int [n] | float [6 m] | float [m] | int | neat_parse_group's own workspace of (n, m)
struct PostRefineWs { int *label, *idx; float *glines, *gscores; int* gcount; void* group; size_t total; };
inline bool post_refine_layout(void* ws, long long n, long long mmax, int parse_tile, PostRefineWs* w) {
  ParseGroupWs g;
  if (!post_counts_ok(n, 1, mmax) || !parse_group_layout(nullptr, (int)n, (int)mmax, parse_tile, &g)) return false;
  WsCarver c(ws);
  w->label = c.take<int>(2 * (size_t)n);
  w->idx = c.take<int>((size_t)n);
  w->glines = c.take<float>(6 * (size_t)mmax);
  w->gscores = c.take<float>((size_t)mmax);
  w->gcount = c.take<int>(1);
  w->group = c.take<char>(g.total);
  w->total = c.end();
  return true;
}

// snap, M = 2 n end points: box float [9] | counts int [2] (cells, peaks) | key, skey, head, flag, cnt, pidx, near int [M] each |
// dist2 float [M] | idx int [n] | pkey, spkey 64-bit [n] each | the sorts' temporary storage: sort_scratch_bytes of the larger list, M
struct PostSnapWs {
  float* box; int *counts, *key, *skey, *head, *flag, *cnt, *pidx, *near; float* dist2; int* idx; unsigned long long *pkey, *spkey; void* sort;
  size_t sort_bytes, total;
};
inline bool post_snap_layout(void* ws, long long n, long long G, PostSnapWs* w) {
  if (!post_grid_ok(G) || !post_counts_ok(n, 1, 0)) return false;
  const size_t M = 2 * (size_t)n;
  w->sort_bytes = sort_scratch_bytes(2 * n);
  WsCarver c(ws);
  w->box = c.take<float>(9);
  w->counts = c.take<int>(2);
  for (int** p : {&w->key, &w->skey, &w->head, &w->flag, &w->cnt, &w->pidx, &w->near}) *p = c.take<int>(M);
  w->dist2 = c.take<float>(M);
  w->idx = c.take<int>((size_t)n);
  w->pkey = c.take<unsigned long long>((size_t)n);
  w->spkey = c.take<unsigned long long>((size_t)n);
  w->sort = c.take<char>(w->sort_bytes);
  w->total = c.end();
  return true;
}

// ---- ray casting: two buffers.  The tree: the status word, the boxes [2 L][6] of a heap of L = 2^k >= max(nf, 1) leaves, the sorted
// triangles [nf][tri_stride].  The build's scratch: Morton keys and face ids with their sorted twins, the per-workgroup boxes (wg faces
// each), the scene box, and the radix sort's room (sort_scratch_bytes)
constexpr int RC_MAX_FACES = 1 << 24;
struct RaycastWs {
  int L, per, tiles;
  int* status; float* nodes; double* tris; size_t bvh_total;
  unsigned long long *key, *skey; int *val, *sval; double *partial, *box; void* sort; size_t sort_bytes, ws_total;
};
inline bool raycast_layout(void* bvh, void* ws, int nf, int wg, int tri_stride, RaycastWs* w) {
  if (nf < 0 || nf > RC_MAX_FACES) return false;
  w->L = 1;
  while (w->L < nf) w->L <<= 1;
  w->per = w->L < wg ? w->L : wg;
  w->tiles = (nf + wg - 1) / wg;
  WsCarver b(bvh);
  w->status = b.take<int>(1);
  w->nodes = b.take<float>((size_t)2 * w->L * 6);
  w->tris = b.take<double>((size_t)nf * tri_stride);
  w->bvh_total = b.end();
  w->sort_bytes = sort_scratch_bytes(nf);
  WsCarver c(ws);
  w->key = c.take<unsigned long long>((size_t)nf);
  w->skey = c.take<unsigned long long>((size_t)nf);
  w->val = c.take<int>((size_t)nf);
  w->sval = c.take<int>((size_t)nf);
  w->partial = c.take<double>((size_t)w->tiles * 6);
  w->box = c.take<double>(6);
  w->sort = c.take<char>(w->sort_bytes);
  w->ws_total = c.end();
  return true;
}

// ---- 2-D line-segment detection (kernels_detect.hpp).  The labelling alone: nothing but the caller's label map.  The detector, over
// px = V Hs Ws grey pixels (Hs = ceil(scale H)), el = V h w gradient positions (h = Hs - 1) and 2 el map elements (view-major, then
// partition): grey [px] first, at offset 0 (detect.py reads it back for the tests), gx, gy [el] | codes byte [2 el] | label, size, votes,
// xmin, xmax, ymax int [2 el] each | per-workgroup counts and offsets [blocks], blocks = ceil(2 el / wg) | counters int [2] (candidates,
// lines) | the candidates: element int [cap], 6 doubles, n, k, keep each [cap] | idx int [cap].  cap = 2 V (h w / min_reg) + 1: a
// candidate region has min_reg pixels at least and the regions of a map are disjoint.
inline bool detect_scale_ok(double scale) { return scale > 0.0 && scale <= 1.0; }
inline int detect_scaled(int size, double scale) {      // ceil(scale size) in float64, as tests/detect_f64.py
  const double s = scale * (double)size;
  long long c = (long long)s;
  if ((double)c < s) ++c;
  return (int)c;
}
inline bool detect_maps_ok(long long maps, long long h, long long w, int tile) {
  if (maps < 0 || h < 0 || w < 0) return false;
  const long long tiles = ((h + tile - 1) / tile) * ((w + tile - 1) / tile);
  return h * w <= 0x7fffffffLL && maps * h * w <= 0x7fffffffLL && maps * tiles <= 0x7fffffffLL;
}
struct DetectWs {
  int Hs, Ws, h, w, blocks, cap;
  long long px, el;
  double *grey, *gx, *gy; unsigned char* code; int *label, *size, *votes, *xmin, *xmax, *ymax, *bcnt, *boff, *counters;
  int* cand; double* rec; int *n, *k, *keep, *idx;
  size_t total;
};
inline bool detect_layout(void* ws, int V, int H, int W, double scale, int min_reg, int tile, int wg, DetectWs* d) {
  if (V < 0 || !detect_scale_ok(scale) || min_reg < 1 || (V > 0 && (H < 2 || W < 2)) || H > 32768 || W > 32768) return false;
  d->Hs = V > 0 ? detect_scaled(H, scale) : 0;
  d->Ws = V > 0 ? detect_scaled(W, scale) : 0;
  d->h = d->Hs > 1 ? d->Hs - 1 : 0;
  d->w = d->Ws > 1 ? d->Ws - 1 : 0;
  if (!detect_maps_ok(2ll * V, d->h, d->w, tile) || (long long)V * d->Hs * d->Ws > 0x7fffffffLL) return false;
  d->px = (long long)V * d->Hs * d->Ws;
  d->el = (long long)V * d->h * d->w;
  d->blocks = (int)((2 * d->el + wg - 1) / wg);
  d->cap = (int)(2ll * V * (((long long)d->h * d->w) / min_reg) + 1);
  const size_t el = (size_t)d->el, cap = (size_t)d->cap;
  WsCarver c(ws);
  d->grey = c.take<double>((size_t)d->px);
  d->gx = c.take<double>(el);
  d->gy = c.take<double>(el);
  d->code = c.take<unsigned char>(2 * el);
  for (int** p : {&d->label, &d->size, &d->votes, &d->xmin, &d->xmax, &d->ymax}) *p = c.take<int>(2 * el);
  d->bcnt = c.take<int>((size_t)d->blocks);
  d->boff = c.take<int>((size_t)d->blocks);
  d->counters = c.take<int>(2);
  d->cand = c.take<int>(cap);
  d->rec = c.take<double>(6 * cap);
  for (int** p : {&d->n, &d->k, &d->keep, &d->idx}) *p = c.take<int>(cap);
  d->total = c.end();
  return true;
}

// ---- triangulation of the views' 2-D segments (kernels_triangulate.hpp) over V views, S segments in all (nmax in one view at most) and
// M neighbour slots.  Every region is bounded by S; the hypothesis list, whose length only the count pass knows, is the caller's.
// sega [9 S] (d_1, d_2, n_a), segb [10 S] (pi, q_1, u, u.u, |pi_xyz|) | cnt, off [S M] (hypotheses per (segment, slot), their offsets) |
// best [S] (the picked hypothesis) | radius [S] | per component, at its root: nviews, axis, last [S] int, tau [2 S] | idx [S] (the kept
// roots in order)
constexpr int TRI_MAX_VIEWS = 65535;
inline bool tri_counts_ok(long long V, long long S, long long M, long long nmax, int tile) {
  if (V < 0 || S < 0 || M < 0 || nmax < 0 || V > TRI_MAX_VIEWS || nmax > S || S > 0x7fffffffLL / 10) return false;
  if (M > 0 && (M >= V || S > 0x7fffffffLL / M)) return false;
  return V * M * ((nmax + tile - 1) / tile) <= 0x7fffffffLL;
}
struct TriWs {
  int tiles;                // tiles of one view in the pair launch: ceil(nmax / tile)
  double *sega, *segb; int *cnt, *off, *best; double* radius; int *nviews, *axis, *last; double* tau; int* idx;
  size_t total;
};
inline bool tri_layout(void* ws, int V, int S, int M, int nmax, int tile, TriWs* w) {
  if (!tri_counts_ok(V, S, M, nmax, tile)) return false;
  w->tiles = (nmax + tile - 1) / tile;
  const size_t s = (size_t)S;
  WsCarver c(ws);
  w->sega = c.take<double>(9 * s);
  w->segb = c.take<double>(10 * s);
  w->cnt = c.take<int>(s * (size_t)M);
  w->off = c.take<int>(s * (size_t)M);
  w->best = c.take<int>(s);
  w->radius = c.take<double>(s);
  for (int** p : {&w->nviews, &w->axis, &w->last}) *p = c.take<int>(s);
  w->tau = c.take<double>(2 * s);
  w->idx = c.take<int>(s);
  w->total = c.end();
  return true;
}

// ---- scene generation (kernels_scenegen.hpp): the visible runs of E edges in V views.  edges [2 E] (the host's list, checked there and
// copied in by the count call) | cnt, off [V E] (runs kept per (view, edge), their offsets).  The run list, whose length only the count
// pass knows, is the caller's.  The picture bounds: one launch over every 16 x 16 tile of every view
constexpr int SG_MAX_VIEWS = 65535;
inline bool scenegen_counts_ok(long long V, long long E) {
  return V >= 0 && E >= 0 && V <= SG_MAX_VIEWS && E <= 0x7fffffffLL / 8 && V * E <= 0x7fffffffLL / 4;
}
inline bool scenegen_picture_ok(long long V, long long H, long long W) {
  if (V < 0 || V > SG_MAX_VIEWS || H < 1 || W < 1 || H > 32768 || W > 32768) return false;
  return V * ((H + 15) / 16) * ((W + 15) / 16) <= 0x7fffffffLL;
}
struct ScenegenWs { int *edges, *cnt, *off; size_t total; };
inline bool scenegen_layout(void* ws, int V, int E, ScenegenWs* w) {
  if (!scenegen_counts_ok(V, E)) return false;
  const size_t pairs = (size_t)V * (size_t)E;
  WsCarver c(ws);
  w->edges = c.take<int>(2 * (size_t)E);
  w->cnt = c.take<int>(pairs);
  w->off = c.take<int>(pairs);
  w->total = c.end();
  return true;
}

// ---- crease lines of a mesh (kernels_crease.hpp): one workspace for the three calls, fixed by (nv, nf) alone.  M = 3 nf bounds the
// half-edges, the feature edges E, the chains and the lines; N = max(nv, 2 M) bounds every sort (vertices, half-edges, 2 E incidences).
// state: two status words, the half-edges kept, then chains, E, lines and junctions as the calls left them | ka, kb, va, vb [N] the
// sorts' keys and values, in and out | per vertex: weld, vhead, vslot, rep (the weld), vstate, jflag, jmap | fn [nf][4] | mark, slot [M]
// (flags and their scans: kinds, then chain heads) | elo, ehi, ekind, parent [M] | ckey [M] the edges in chain order, cstart [M + 1],
// cinfo [M][4], cnl, coff [M] | lab, ltag [M] the lines before their sort | tile: the scans' tile sums | the radix sort's room
// (sort_scratch_bytes)
constexpr int CR_MAX_VERTS = 1 << 26;
struct CreaseWs {
  int M; size_t N;
  int* state; unsigned long long *ka, *kb; int *va, *vb;
  int *weld, *vhead, *vslot, *rep, *vstate, *jflag, *jmap;
  double* fn; int *mark, *slot, *elo, *ehi, *ekind, *parent;
  unsigned long long* ckey; int *cstart, *cinfo, *cnl, *coff;
  unsigned long long* lab; int *ltag, *tile; void* sort; size_t sort_bytes, total;
};
inline bool crease_layout(void* ws, int nv, int nf, int scan_tile, CreaseWs* w) {
  if (nv < 0 || nf < 0 || nv > CR_MAX_VERTS || nf > RC_MAX_FACES) return false;
  w->M = 3 * nf;
  const size_t M = (size_t)w->M, V = (size_t)nv;
  w->N = V > 2 * M ? V : 2 * M;
  w->sort_bytes = sort_scratch_bytes((long long)w->N);
  WsCarver c(ws);
  w->state = c.take<int>(64);
  w->ka = c.take<unsigned long long>(w->N);
  w->kb = c.take<unsigned long long>(w->N);
  w->va = c.take<int>(w->N);
  w->vb = c.take<int>(w->N);
  for (int** p : {&w->weld, &w->vhead, &w->vslot, &w->rep, &w->vstate, &w->jflag, &w->jmap}) *p = c.take<int>(V);
  w->fn = c.take<double>(4 * (size_t)nf);
  for (int** p : {&w->mark, &w->slot, &w->elo, &w->ehi, &w->ekind, &w->parent}) *p = c.take<int>(M);
  w->ckey = c.take<unsigned long long>(M);
  w->cstart = c.take<int>(M + 1);
  w->cinfo = c.take<int>(4 * M);
  w->cnl = c.take<int>(M);
  w->coff = c.take<int>(M);
  w->lab = c.take<unsigned long long>(M);
  w->ltag = c.take<int>(M);
  w->tile = c.take<int>(w->N / (size_t)scan_tile + 1);
  w->sort = c.take<char>(w->sort_bytes);
  w->total = c.end();
  return true;
}

// ---- 2-D wireframes with shared junctions (kernels_wireframe2d.hpp) over V views, S segments in all, nmax in one view at most (an upper
// bound will do: it sizes the pair launches' grid).  Every region is bounded by S.  rec [8 S] (p, q, u, L, g) | view [S] | per endpoint:
// parent (then the label), last (a root's highest member), vidx (a root's place in the vertex list) [2 S] each | keep, eidx [S] (a
// segment is an edge; the edges before it)
constexpr int WF_MAX_VIEWS = 65535;
inline bool wf2d_counts_ok(long long V, long long S, long long nmax, int tile) {
  if (V < 0 || S < 0 || nmax < 0 || V > WF_MAX_VIEWS || nmax > S || S > 0x7fffffffLL / 10 || (S > 0 && (V == 0 || nmax == 0))) return false;
  return V * ((nmax + tile - 1) / tile) <= 0x7fffffffLL;
}
struct Wf2dWs {
  int tiles;                // tiles of one view in the pair launches: ceil(nmax / tile)
  double* rec; int *view, *parent, *last, *vidx, *keep, *eidx;
  size_t total;
};
inline bool wf2d_layout(void* ws, int V, int S, int nmax, int tile, Wf2dWs* w) {
  if (!wf2d_counts_ok(V, S, nmax, tile)) return false;
  w->tiles = (nmax + tile - 1) / tile;
  const size_t s = (size_t)S;
  WsCarver c(ws);
  w->rec = c.take<double>(8 * s);
  w->view = c.take<int>(s);
  for (int** p : {&w->parent, &w->last, &w->vidx}) *p = c.take<int>(2 * s);
  w->keep = c.take<int>(s);
  w->eidx = c.take<int>(s);
  w->total = c.end();
  return true;
}

// ---- 3-D wireframes with shared junctions (kernels_wireframe3d.hpp) over V views, S 2-D segments, N 3-D lines, NV 2-D vertices and room
// for pairs_max pair keys.  An end id is below 2 N < 2^24 and a view below 2^16, so a pair key (24 + 24 + 16 bits) fits 64 bits.
// total: the pairs there are | rkey, rskey [2 S] the records and their sort | rcnt [2 S], roff [2 S] the pairs a record starts and
// those before it | vview [NV] | pkey, pskey [pairs_max] | per end id: parent (then the label), last, vidx, lvotes [2 N] each | per line:
// ekey, eskey, eline, esline (the edge keys and their sort), keep, eidx [N] | the radix sort's room (sort_scratch_bytes)
constexpr int WF3_MAX_ENDS = 1 << 24;
inline bool wf3d_counts_ok(long long V, long long S, long long N, long long NV, long long pairs_max) {
  if (V < 0 || S < 0 || N < 0 || NV < 0 || pairs_max < 0 || V > WF_MAX_VIEWS || 2 * N >= WF3_MAX_ENDS) return false;
  return 6 * S <= 0x7fffffffLL && NV <= 0x7fffffffLL && pairs_max <= 0x7fffffffLL && (S == 0 || (V > 0 && NV > 0));
}
struct Wf3dWs {
  size_t n_sort;            // the largest list a sort sees
  long long* total; unsigned long long *rkey, *rskey; int* rcnt; long long* roff; int* vview;
  unsigned long long *pkey, *pskey; int *parent, *last, *vidx, *lvotes;
  unsigned long long *ekey, *eskey; int *eline, *esline, *keep, *eidx;
  void* sort; size_t sort_bytes, total_bytes;
};
inline bool wf3d_layout(void* ws, int V, int S, int N, int NV, long long pairs_max, Wf3dWs* w) {
  if (!wf3d_counts_ok(V, S, N, NV, pairs_max)) return false;
  const size_t s2 = 2 * (size_t)S, n = (size_t)N, p = (size_t)pairs_max;
  w->n_sort = s2 > p ? (s2 > n ? s2 : n) : (p > n ? p : n);
  w->sort_bytes = sort_scratch_bytes((long long)w->n_sort);
  WsCarver c(ws);
  w->total = c.take<long long>(32);
  w->rkey = c.take<unsigned long long>(s2);
  w->rskey = c.take<unsigned long long>(s2);
  w->rcnt = c.take<int>(s2);
  w->roff = c.take<long long>(s2);
  w->vview = c.take<int>((size_t)NV);
  w->pkey = c.take<unsigned long long>(p);
  w->pskey = c.take<unsigned long long>(p);
  for (int** q : {&w->parent, &w->last, &w->vidx, &w->lvotes}) *q = c.take<int>(2 * n);
  w->ekey = c.take<unsigned long long>(n);
  w->eskey = c.take<unsigned long long>(n);
  for (int** q : {&w->eline, &w->esline, &w->keep, &w->eidx}) *q = c.take<int>(n);
  w->sort = c.take<char>(w->sort_bytes);
  w->total_bytes = c.end();
  return true;
}

}  // namespace neat
