// Stand-alone check of neat_amd/csrc/ws_layout.hpp (the carver, every workspace layout, the count bounds) under the host sanitizers.
// No device is touched.  Build and run (host code only is instrumented):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Ineat_amd/csrc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         scripts/ws_host_check.cpp -o /tmp/ws_host_check && /tmp/ws_host_check
// Each layout is measured over a null base (regions in order, disjoint, aligned as declared, at least as large as what the kernels
// index), then carved from an allocation of exactly the reported size, where every region is filled to the extent the kernels index:
// a region past the total is a heap overflow the address sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernels_detect.hpp"
#include "kernels_evalmesh.hpp"
#include "kernels_frame.hpp"
#include "kernels_mesh.hpp"
#include "kernels_parse.hpp"
#include "kernels_raycast.hpp"
#include "kernels_show.hpp"
#include "kernels_trace.hpp"
#include "kernels_triangulate.hpp"
#include "kernels_wireframe2d.hpp"
#include "ws_layout.hpp"

using namespace neat;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct Region { const void* p; size_t need, align; };
typedef std::vector<Region> Regions;

// fill(base, regions, total) runs one layout over `base` and lists its regions with the bytes the kernels index and the declared alignment
template <class F>
static bool layout_ok(F fill, size_t total_align = 256) {
  Regions m, r;
  size_t total = 0, total2 = 0;
  if (!fill((void*)nullptr, m, total) || total % total_align != 0) return false;
  std::vector<size_t> off;
  for (const Region& g : m) off.push_back(ws_offset(nullptr, g.p));
  for (size_t i = 0; i < m.size(); ++i) {
    const size_t end = i + 1 < m.size() ? off[i + 1] : total;
    if (off[i] % m[i].align != 0 || end < off[i] || end - off[i] < m[i].need) return false;
  }
  if (total > ((size_t)256 << 20)) return true;              // the large cases are measured only
  char* base = (char*)std::malloc(total ? total : 1);
  bool ok = fill((void*)base, r, total2) && total2 == total && r.size() == m.size();
  for (size_t i = 0; ok && i < r.size(); ++i) {
    ok = r[i].p == base + off[i];
    if (ok && r[i].need) std::memset(const_cast<void*>(r[i].p), 0xab, r[i].need);
  }
  std::free(base);
  return ok;
}

static const long long COUNTS[] = {0, 1, 255, 256, 257, 50000};

int main() {
  // the carver
  CHECK(ws_align(0) == 0 && ws_align(1) == 256 && ws_align(256) == 256 && ws_align(257) == 512 && ws_align(9, 8) == 16 && ws_align(8, 4) == 8);
  {
    WsCarver c(nullptr);
    CHECK(ws_offset(nullptr, c.take<double>(3, 8)) == 0 && ws_offset(nullptr, c.take<int>(1, 4)) == 24 && c.end(4) == 28);
    CHECK(ws_offset(nullptr, c.take<char>(0)) == 256 && c.end() == 256 && ws_offset(nullptr, c.take<long long>(2, 8)) == 256 && c.end(8) == 272);
  }
  // the radix sort's room: nothing for an empty list, 32 bytes an element and 4 MiB otherwise, no wrap at the largest list
  CHECK(sort_scratch_bytes(-1) == 0 && sort_scratch_bytes(0) == 0 && sort_scratch_bytes(1) == 32 + ((size_t)4 << 20));
  CHECK(sort_scratch_bytes(4097) == 32 * (size_t)4097 + ((size_t)4 << 20) && sort_scratch_bytes(0x7fffffffLL) == 32 * (size_t)0x7fffffff + ((size_t)4 << 20));
  // count bounds
  CHECK(post_counts_ok(0, 0, 0) && post_counts_ok(50000, 64, 32000) && post_counts_ok(0x7fffffffLL / 6, 1, 0));
  CHECK(!post_counts_ok(-1, 1, 1) && !post_counts_ok(1, -1, 1) && !post_counts_ok(1, 1, -1));
  CHECK(!post_counts_ok(0x7fffffffLL / 6 + 1, 1, 0) && !post_counts_ok(10, POST_MAX_VIEWS + 1, 0));
  CHECK(!post_counts_ok(0x7fffffffLL / 6, 7, 0));                          // n V beyond an int
  CHECK(post_grid_ok(2) && post_grid_ok(512) && post_grid_ok(1024) && !post_grid_ok(1) && !post_grid_ok(1025) && !post_grid_ok(2048) &&
        !post_grid_ok(-4));
  CHECK((long long)(POST_MAX_GRID - 1) * POST_MAX_GRID * POST_MAX_GRID + (long long)(POST_MAX_GRID - 1) * POST_MAX_GRID + POST_MAX_GRID - 1 <
        (1LL << 30));                                                       // the largest cell key

  for (long long n : COUNTS) {
    // ---- post
    for (long long V : {0LL, 1LL, 3LL, 64LL}) {
      for (long long mt : {0LL, 1LL, 1025LL, 32000LL}) {
        CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
          PostFuseWs w;
          if (!post_fuse_layout(b, n, V, mt, &w)) return false;
          r = {{w.label, (size_t)(n * V * 4), 256}, {w.present, (size_t)mt, 256}, {w.rank, (size_t)(mt * 4), 256}, {w.idx, (size_t)(n * 4), 256}};
          t = w.total;
          return true;
        }));
      }
    }
    for (long long mm : {0LL, 1LL, 500LL}) {
      ParseGroupWs g;
      CHECK(parse_group_layout(nullptr, (int)n, (int)mm, PARSE_TILE, &g));
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        PostRefineWs w;
        if (!post_refine_layout(b, n, mm, PARSE_TILE, &w)) return false;
        r = {{w.label, (size_t)(8 * n), 256}, {w.idx, (size_t)(4 * n), 256}, {w.glines, (size_t)(24 * mm), 256}, {w.gscores, (size_t)(4 * mm), 256},
             {w.gcount, sizeof(int), 256}, {w.group, g.total, 256}};
        t = w.total;
        return true;
      }));
    }
    for (long long G : {2LL, 8LL, 512LL, 1024LL}) {
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        PostSnapWs w;
        if (!post_snap_layout(b, n, G, &w) || w.sort_bytes != sort_scratch_bytes(2 * n)) return false;
        const size_t M4 = (size_t)(8 * n);
        r = {{w.box, 36, 256}, {w.counts, 8, 256}, {w.key, M4, 256}, {w.skey, M4, 256}, {w.head, M4, 256}, {w.flag, M4, 256}, {w.cnt, M4, 256},
             {w.pidx, M4, 256}, {w.near, M4, 256}, {w.dist2, M4, 256}, {w.idx, (size_t)(4 * n), 256}, {w.pkey, (size_t)(8 * n), 256},
             {w.spkey, (size_t)(8 * n), 256}, {w.sort, w.sort_bytes, 256}};
        t = w.total;
        return true;
      }));
    }
    PostSnapWs ws;
    CHECK(!post_snap_layout(nullptr, n, 2048, &ws) && !post_snap_layout(nullptr, n, 1, &ws));

    // ---- lsap (n rows against 1, 8 and n columns; float64 first, 8-byte aligned; ints behind them, 4-byte aligned), dbscan
    for (long long nc : {1LL, 8LL, n}) {
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        LsapWs w;
        lsap_layout(b, (int)n, (int)nc, &w);
        const size_t mx = (size_t)(n > nc ? n : nc), mn = (size_t)(n < nc ? n : nc);
        r = {{w.d, (mn + 2 * mx) * 8, 8}, {w.i, ((size_t)n + (size_t)nc + 5 * mx + 2 * mn) * 4, 4}};      // u, v, sp | the eight int arrays of LsapArgs
        t = w.total;
        return true;
      }, 4));
    }
    CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
      DbscanWs w;
      dbscan_layout(b, (int)n, &w);
      r = {{w.parent, (size_t)(4 * n), 4}, {w.has_nb, (size_t)(4 * n), 4}};
      t = w.total;
      return true;
    }, 4));

    // ---- parse
    for (int m : {0, 1, 257}) {
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        ParseGroupWs w;
        if (!parse_group_layout(b, (int)n, m, PARSE_TILE, &w)) return false;
        if ((long long)w.tiles * PARSE_TILE < 2 * n) return false;                  // the tiles cover the 2 n rows
        const size_t m4 = (size_t)m * 4;
        r = {{w.run, (size_t)w.tiles * m4, 256}, {w.cnt, m4, 4}, {w.start, m4, 4}, {w.slot, m4, 4}, {w.order, (size_t)(8 * n), 256}};
        t = w.total;
        return true;
      }));
    }
    for (int mcap : {1, 128, 257}) {
      if (n == 0) continue;
      LsapWs l;
      lsap_layout(nullptr, (int)n, 2 * mcap, &l);
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        ParseVoteWs w;
        if (!parse_vote_layout(b, (int)n, mcap, &w)) return false;
        if (w.nc != 2 * mcap || w.k != (n < 2 * mcap ? n : 2 * mcap)) return false;
        r = {{w.cost, (size_t)(n * w.nc * 4), 256}, {w.cmask, (size_t)w.nc, 256}, {w.rows, (size_t)w.k * 8, 256}, {w.cols, (size_t)w.k * 8, 256},
             {w.n_match, 4, 256}, {w.lsap, l.total, 256}};
        t = w.total;
        return true;
      }));
    }
    for (int V : {0, 1, 3}) {
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        ParseGraphWs w;
        if (!parse_graph_layout(b, V, (int)n, 257, &w)) return false;
        r = {{w.idx, (size_t)(V * n * 4), 256}, {w.rowcnt, 257 * 4, 256}};
        t = w.total;
        return true;
      }));
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        ParseVisWs w;
        if (!parse_vis_layout(b, (int)n, V, &w)) return false;
        r = {{w.vis, (size_t)(V * n), 256}, {w.idx, (size_t)(4 * n), 256}};
        t = w.total;
        return true;
      }));
    }

    // ---- mesh: 2 x 2 x (n + 2) nodes
    CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
      MeshWs w;
      if (!mesh_layout(b, 2, 2, (int)n + 2, MESH_TILE, &w)) return false;
      if (w.nodes != 4 * (n + 2) || (long long)w.tiles * MESH_TILE < w.nodes || (long long)(w.tiles - 1) * MESH_TILE >= w.nodes) return false;
      r = {{w.emask, (size_t)w.nodes, 256}, {w.vbase, (size_t)w.nodes * 4, 256}, {w.tile_v, (size_t)w.tiles * 4, 256}, {w.tile_f, (size_t)w.tiles * 4, 256}};
      t = w.total;
      return true;
    }));

    // ---- the sum trees: n 1024 + 1 inputs reach the levels above the leaves; every level holds its [comps][m] sums and ends in one value
    for (int tree = 0; tree < 2; ++tree) {
      const int leaf = tree ? FRAME_WG : MOMENTS_TILE, fan = tree ? FRAME_WG : EMESH_WG, comps = tree ? 1 : MOMENTS_N;
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        SumTreeWs w;
        const long long items = n * 1024 + 1;
        if (!sum_tree_layout(b, items, leaf, fan, comps, &w) || w.levels > 8 || w.m[w.levels] != 1 || w.level[w.levels]) return false;
        long long m = (items + leaf - 1) / leaf;
        for (int k = 0; k < w.levels; ++k, m = (m + fan - 1) / fan) {
          if (w.m[k] != m || m <= 1) return false;
          r.push_back({w.level[k], (size_t)comps * (size_t)m * 8, 8});
        }
        if (m != 1) return false;
        t = w.total;
        return true;
      }));
    }

    // ---- evaluation
    for (int buckets : {1, 255, 256, 257, 1331}) {
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        EvalGridWs w;
        if (!eval_grid_layout(b, (int)n, buckets, &w)) return false;
        r = {{w.cnt, (size_t)buckets * 4, 256}, {w.bucket_of, (size_t)(4 * n), 256}};
        t = w.total;
        return true;
      }));
    }
    CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
      EvalTriWs w;
      if (!eval_tri_layout(b, (int)n, &w)) return false;
      r = {{w.counts, (size_t)(4 * n), 256}, {w.offs, (size_t)(4 * (n + 1)), 256}};      // eval_exscan_kernel writes out[0 .. nf]
      t = w.total;
      return true;
    }));

    // ---- pictures: one frame of (n + 1) x 3 pixels
    CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
      ShowWs s;
      if (!show_layout(b, 1, (int)n % 32768 + 1, 3, SHOW_QUEUE_CAP, &s)) return false;
      const size_t px = (size_t)s.pixels;
      if (ws_offset(s.status, s.queued) != 8 || ws_offset(s.status, s.queue) != 256) return false;
      r = {{s.key, px * 8, 256}, {s.cov, px * 4, 256}, {s.covp, px * 4, 256}, {s.status, 4, 256}, {s.queued, 8, 8}, {s.queue, (size_t)SHOW_QUEUE_CAP * 8, 256}};
      t = s.total;
      return true;
    }, 8));

    // ---- trace
    if (n >= 1) {
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        TraceWs w;
        if (!(t = trace_layout(b, (int)n, TRACE_WG, &w))) return false;
        const size_t f = (size_t)(4 * n), tiles = (size_t)((n + TRACE_WG - 1) / TRACE_WG);
        r = {{w.t, f, 256}, {w.ta, f, 256}, {w.fa, f, 256}, {w.tb, f, 256}, {w.fb, f, 256}, {w.t1, f, 256}, {w.steps, f, 256}, {w.march, f, 256},
             {w.refine, f, 256}, {w.ids[0], f, 256}, {w.ids[1], f, 256}, {w.phase, (size_t)n, 256}, {w.side, (size_t)n, 256}, {w.flag, (size_t)n, 256},
             {w.tile, tiles * 4, 256}};
        return true;
      }));
    }

    // ---- ray casting: the tree and the build's scratch
    for (int buffer = 0; buffer < 2; ++buffer) {
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        RaycastWs w;
        if (!raycast_layout(buffer ? nullptr : b, buffer ? b : nullptr, (int)n, RC_WG, RC_TRI_STRIDE, &w)) return false;
        if (w.L < (n > 1 ? n : 1) || (w.L & (w.L - 1)) || (w.L > 1 && w.L / 2 >= n) || w.per != (w.L < RC_WG ? w.L : RC_WG)) return false;
        if ((long long)w.tiles * RC_WG < n) return false;
        if (buffer == 0) {
          r = {{w.status, 4, 256}, {w.nodes, (size_t)w.L * 48, 256}, {w.tris, (size_t)(n * RC_TRI_STRIDE * 8), 256}};
          t = w.bvh_total;
        } else {
          r = {{w.key, (size_t)(8 * n), 256}, {w.skey, (size_t)(8 * n), 256}, {w.val, (size_t)(4 * n), 256}, {w.sval, (size_t)(4 * n), 256},
               {w.partial, (size_t)w.tiles * 48, 256}, {w.box, 48, 256}, {w.sort, w.sort_bytes, 256}};
          t = w.ws_total;
        }
        return true;
      }));
    }
  }

  // ---- line-segment detection: pictures around the labelling's tile (gradient grids of 15, 16, 17) and one scaled down
  {
    const int shapes[][3] = {{0, 0, 0}, {1, 2, 2}, {1, 16, 16}, {1, 17, 17}, {3, 18, 33}, {2, 97, 131}, {8, 128, 128}};
    for (const auto& sh : shapes)
      for (double scale : {1.0, 0.8})
        for (int min_reg : {1, 12}) {
          CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
            DetectWs d;
            if (!detect_layout(b, sh[0], sh[1], sh[2], scale, min_reg, DET_TILE, DET_WG, &d)) return false;
            const size_t el = (size_t)d.el, cap = (size_t)d.cap;
            if (d.h != (d.Hs > 1 ? d.Hs - 1 : 0) || d.el != (long long)sh[0] * d.h * d.w || (long long)d.blocks * DET_WG < 2 * d.el) return false;
            if (ws_offset(b, d.grey) != 0 || cap < 1 || (long long)cap * min_reg < 2 * d.el - 2ll * sh[0] * (min_reg - 1)) return false;
            r = {{d.grey, (size_t)d.px * 8, 256}, {d.gx, el * 8, 256}, {d.gy, el * 8, 256}, {d.code, 2 * el, 256}, {d.label, 8 * el, 256},
                 {d.size, 8 * el, 256}, {d.votes, 8 * el, 256}, {d.xmin, 8 * el, 256}, {d.xmax, 8 * el, 256}, {d.ymax, 8 * el, 256},
                 {d.bcnt, (size_t)d.blocks * 4, 256}, {d.boff, (size_t)d.blocks * 4, 256}, {d.counters, 8, 256}, {d.cand, cap * 4, 256},
                 {d.rec, cap * 48, 256}, {d.n, cap * 4, 256}, {d.k, cap * 4, 256}, {d.keep, cap * 4, 256}, {d.idx, cap * 4, 256}};
            t = d.total;
            return true;
          }));
        }
    CHECK(detect_scaled(128, 0.8) == 103 && detect_scaled(5, 0.8) == 4 && detect_scaled(10, 1.0) == 10 && detect_scaled(2, 0.3) == 1);
  }

  // ---- triangulation: views, segments in all, neighbour slots, the largest view; segment counts around the pair kernel's tile
  {
    const int shapes[][4] = {{0, 0, 0, 0}, {1, 5, 0, 5}, {2, 1, 1, 1}, {3, 255, 2, 255}, {3, 600, 2, 256}, {7, 761, 6, 257}, {64, 32000, 10, 500}};
    for (const auto& sh : shapes) {
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        TriWs w;
        if (!tri_layout(b, sh[0], sh[1], sh[2], sh[3], TRI_WG, &w)) return false;
        const size_t s = (size_t)sh[1], sm = s * (size_t)sh[2];
        if ((long long)w.tiles * TRI_WG < sh[3] || (w.tiles > 0 && (long long)(w.tiles - 1) * TRI_WG >= sh[3])) return false;
        r = {{w.sega, s * TRI_SEGA * 8, 256}, {w.segb, s * TRI_SEGB * 8, 256}, {w.cnt, sm * 4, 256}, {w.off, sm * 4, 256}, {w.best, s * 4, 256},
             {w.radius, s * 8, 256}, {w.nviews, s * 4, 256}, {w.axis, s * 4, 256}, {w.last, s * 4, 256}, {w.tau, s * 16, 256}, {w.idx, s * 4, 256}};
        t = w.total;
        return true;
      }));
    }
    CHECK(tri_counts_ok(64, 32000, 10, 500, TRI_WG) && tri_counts_ok(0, 0, 0, 0, TRI_WG) && tri_counts_ok(TRI_MAX_VIEWS, 100000, 6, 10, TRI_WG));
    CHECK(TRI_WG * TRI_SEGB * 8 <= 64 * 1024);                             // the pair kernel's tile of partners in LDS
  }

  // ---- 2-D wireframes: views, segments in all, the largest view (or a bound on it); segment counts around the pair kernels' tile
  {
    const int shapes[][3] = {{0, 0, 0}, {1, 1, 1}, {3, 3, 2}, {1, 255, 255}, {1, 256, 256}, {2, 257, 257}, {5, 600, 600}, {64, 128000, 2000}, {64, 128000, 128000}};
    for (const auto& sh : shapes) {
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        Wf2dWs w;
        if (!wf2d_layout(b, sh[0], sh[1], sh[2], WF_WG, &w)) return false;
        const size_t s = (size_t)sh[1];
        if ((long long)w.tiles * WF_WG < sh[2] || (w.tiles > 0 && (long long)(w.tiles - 1) * WF_WG >= sh[2])) return false;
        r = {{w.rec, s * WF_REC * 8, 256}, {w.view, s * 4, 256}, {w.parent, s * 8, 256}, {w.last, s * 8, 256}, {w.vidx, s * 8, 256},
             {w.keep, s * 4, 256}, {w.eidx, s * 4, 256}};
        t = w.total;
        return true;
      }));
    }
    CHECK(wf2d_counts_ok(64, 128000, 2000, WF_WG) && wf2d_counts_ok(0, 0, 0, WF_WG) && wf2d_counts_ok(WF_MAX_VIEWS, 0x7fffffff / 10, 8000, WF_WG));
    CHECK(WF_WG * WF_REC * 8 <= 64 * 1024);                                // the pair kernels' tile of partners in LDS
  }

  // ---- 3-D wireframes: views, 2-D segments, 3-D lines, 2-D vertices, room for pair keys; counts around the workgroup and empty parts
  {
    const long long shapes[][5] = {{0, 0, 0, 0, 0}, {1, 1, 1, 2, 1}, {0, 0, 20, 0, 0}, {4, 80, 0, 60, 16}, {3, 771, 257, 774, 100000},
                                   {12, 150, 17, 140, 4096}, {4, 1024, 256, 400, 255}, {64, 128000, 40000, 90000, 512000}};
    for (const auto& sh : shapes) {
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        Wf3dWs w;
        if (!wf3d_layout(b, (int)sh[0], (int)sh[1], (int)sh[2], (int)sh[3], sh[4], &w)) return false;
        const size_t s2 = 2 * (size_t)sh[1], n = (size_t)sh[2], nv = (size_t)sh[3], p = (size_t)sh[4];
        if (w.n_sort < s2 || w.n_sort < n || w.n_sort < p || w.sort_bytes < 32 * w.n_sort) return false;
        r = {{w.total, 8, 256}, {w.rkey, s2 * 8, 256}, {w.rskey, s2 * 8, 256}, {w.rcnt, s2 * 4, 256}, {w.roff, s2 * 8, 256}, {w.vview, nv * 4, 256},
             {w.pkey, p * 8, 256}, {w.pskey, p * 8, 256}};
        for (int* q : {w.parent, w.last, w.vidx, w.lvotes}) r.push_back({q, 2 * n * 4, 256});
        r.push_back({w.ekey, n * 8, 256});
        r.push_back({w.eskey, n * 8, 256});
        for (int* q : {w.eline, w.esline, w.keep, w.eidx}) r.push_back({q, n * 4, 256});
        r.push_back({w.sort, w.sort_bytes, 256});
        t = w.total_bytes;
        return true;
      }));
    }
    CHECK(wf3d_counts_ok(WF_MAX_VIEWS, 0x7fffffffLL / 6, WF3_MAX_ENDS / 2 - 1, 0x7fffffffLL, 0x7fffffffLL) && wf3d_counts_ok(0, 0, 0, 0, 0));
    CHECK(!wf3d_counts_ok(-1, 0, 0, 0, 0) && !wf3d_counts_ok(1, -1, 0, 1, 0) && !wf3d_counts_ok(1, 1, -1, 1, 0) && !wf3d_counts_ok(1, 1, 1, -1, 0) &&
          !wf3d_counts_ok(1, 1, 1, 1, -1) && !wf3d_counts_ok(WF_MAX_VIEWS + 1, 1, 1, 1, 1) && !wf3d_counts_ok(1, 1, WF3_MAX_ENDS / 2, 1, 1) &&
          !wf3d_counts_ok(1, 0x7fffffffLL / 6 + 1, 1, 1, 1) && !wf3d_counts_ok(1, 1, 1, 0x80000000LL, 1) && !wf3d_counts_ok(1, 1, 1, 1, 0x80000000LL) &&
          !wf3d_counts_ok(0, 1, 1, 1, 1) && !wf3d_counts_ok(1, 1, 1, 0, 1));
    CHECK(2LL * (WF3_MAX_ENDS / 2 - 1) + 1 < (1LL << 24) && WF_MAX_VIEWS < (1 << 16));          // an end id in 24 bits, a view in 16: a pair key in 64
  }

  // ---- scene generation: views and edges; the edge list, then the runs per (view, edge) and their offsets
  {
    const int shapes[][2] = {{0, 0}, {0, 18}, {3, 0}, {1, 1}, {3, 12}, {100, 18}, {7, 257}, {SG_MAX_VIEWS, 4096}};
    for (const auto& sh : shapes) {
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        ScenegenWs w;
        if (!scenegen_layout(b, sh[0], sh[1], &w)) return false;
        const size_t pairs = (size_t)sh[0] * (size_t)sh[1];
        r = {{w.edges, (size_t)sh[1] * 8, 256}, {w.cnt, pairs * 4, 256}, {w.off, pairs * 4, 256}};
        t = w.total;
        return true;
      }));
    }
    CHECK(scenegen_counts_ok(100, 18) && scenegen_counts_ok(0, 0) && scenegen_counts_ok(SG_MAX_VIEWS, 0x7fffffff / 4 / SG_MAX_VIEWS));
    CHECK(scenegen_picture_ok(100, 512, 512) && scenegen_picture_ok(0, 1, 1) && scenegen_picture_ok(SG_MAX_VIEWS, 2048, 2048));
    CHECK((long long)SG_MAX_VIEWS * (2048 / 16) * (2048 / 16) <= 0x7fffffffLL);      // the grid of that launch
  }

  // ---- crease lines: vertices and faces; M = 3 nf half-edges, N = max(nv, 2 M) elements in a sort, tiles of 1024 in a scan
  {
    const int shapes[][2] = {{0, 0}, {1, 1}, {3, 0}, {0, 4}, {255, 256}, {256, 257}, {4097, 4096}, {100000, 7}, {12291, 16388}};
    for (const auto& sh : shapes) {
      CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
        CreaseWs w;
        if (!crease_layout(b, sh[0], sh[1], 1024, &w)) return false;
        const size_t V = (size_t)sh[0], M = 3 * (size_t)sh[1], N = V > 2 * M ? V : 2 * M;
        if (w.N != N || (size_t)w.M != M || w.sort_bytes < 32 * N) return false;
        r = {{w.state, 256, 256}, {w.ka, N * 8, 256}, {w.kb, N * 8, 256}, {w.va, N * 4, 256}, {w.vb, N * 4, 256}};
        for (int* p : {w.weld, w.vhead, w.vslot, w.rep, w.vstate, w.jflag, w.jmap}) r.push_back({p, V * 4, 256});
        r.push_back({w.fn, (size_t)sh[1] * 32, 256});
        for (int* p : {w.mark, w.slot, w.elo, w.ehi, w.ekind, w.parent}) r.push_back({p, M * 4, 256});
        r.push_back({w.ckey, M * 8, 256});
        r.push_back({w.cstart, (M + 1) * 4, 256});
        r.push_back({w.cinfo, M * 16, 256});
        r.push_back({w.cnl, M * 4, 256});
        r.push_back({w.coff, M * 4, 256});
        r.push_back({w.lab, M * 8, 256});
        r.push_back({w.ltag, M * 4, 256});
        r.push_back({w.tile, ((N + 1023) / 1024) * 4, 256});
        r.push_back({w.sort, w.sort_bytes, 256});
        t = w.total;
        return true;
      }));
    }
    CreaseWs wc;
    CHECK(!crease_layout(nullptr, -1, 1, 1024, &wc) && !crease_layout(nullptr, 1, -1, 1024, &wc) && !crease_layout(nullptr, CR_MAX_VERTS + 1, 1, 1024, &wc) &&
          !crease_layout(nullptr, 1, RC_MAX_FACES + 1, 1024, &wc));
    CHECK(crease_layout(nullptr, CR_MAX_VERTS, RC_MAX_FACES, 1024, &wc) && 2 * (long long)wc.M <= 0x7fffffffLL);      // every index is an int
  }

  // the large values: measured only
  CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
    TriWs w;
    if (!tri_layout(b, 1000, 0x7fffffff / 10, 10, 400000, TRI_WG, &w)) return false;
    r = {{w.sega, (size_t)(0x7fffffff / 10) * 72, 256}, {w.cnt, (size_t)(0x7fffffff / 10) * 40, 256}, {w.idx, (size_t)(0x7fffffff / 10) * 4, 256}};
    t = w.total;
    return true;
  }));
  CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
    DetectWs d;
    if (!detect_layout(b, 64, 1200, 1600, 1.0, 18, DET_TILE, DET_WG, &d)) return false;
    r = {{d.grey, (size_t)d.px * 8, 256}, {d.label, (size_t)d.el * 8, 256}, {d.idx, (size_t)d.cap * 4, 256}};
    t = d.total;
    return true;
  }));
  CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
    TraceWs w;
    if (!(t = trace_layout(b, TRACE_MAX_RAYS, TRACE_WG, &w))) return false;
    r = {{w.t, (size_t)4 << 24, 256}, {w.ids[1], (size_t)4 << 24, 256}, {w.flag, (size_t)1 << 24, 256}, {w.tile, (size_t)4 << 16, 256}};
    return true;
  }));
  CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
    MeshWs w;
    if (!mesh_layout(b, 1024, 1024, 2047, MESH_TILE, &w)) return false;
    r = {{w.emask, (size_t)w.nodes, 256}, {w.vbase, (size_t)w.nodes * 4, 256}, {w.tile_v, (size_t)w.tiles * 4, 256}, {w.tile_f, (size_t)w.tiles * 4, 256}};
    t = w.total;
    return true;
  }));
  CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
    RaycastWs w;
    if (!raycast_layout(b, nullptr, RC_MAX_FACES, RC_WG, RC_TRI_STRIDE, &w) || w.L != RC_MAX_FACES) return false;
    r = {{w.status, 4, 256}, {w.nodes, (size_t)w.L * 48, 256}, {w.tris, (size_t)RC_MAX_FACES * RC_TRI_STRIDE * 8, 256}};
    t = w.bvh_total;
    return true;
  }));
  CHECK(layout_ok([&](void* b, Regions& r, size_t& t) {
    ShowWs s;
    if (!show_layout(b, 64, 2048, 2048, SHOW_QUEUE_CAP, &s)) return false;
    r = {{s.key, (size_t)s.pixels * 8, 256}, {s.cov, (size_t)s.pixels * 4, 256}, {s.covp, (size_t)s.pixels * 4, 256}, {s.status, 4, 256}};
    t = s.total;
    return true;
  }, 8));

  // every out-of-range argument set is refused
  PostFuseWs wf;
  CHECK(!post_fuse_layout(nullptr, 0x7fffffffLL, 1, 0, &wf) && !post_fuse_layout(nullptr, 10, 70000, 0, &wf));
  PostRefineWs wr;
  CHECK(!post_refine_layout(nullptr, -1, 1, PARSE_TILE, &wr) && !post_refine_layout(nullptr, 1, -1, PARSE_TILE, &wr));
  PostSnapWs wsn;
  CHECK(!post_snap_layout(nullptr, -1, 8, &wsn));
  ParseGroupWs wg;
  CHECK(!parse_group_layout(nullptr, -1, 1, PARSE_TILE, &wg) && !parse_group_layout(nullptr, 1, -1, PARSE_TILE, &wg));
  ParseVoteWs wv;
  CHECK(!parse_vote_layout(nullptr, 0, 1, &wv) && !parse_vote_layout(nullptr, 1, 0, &wv) && !parse_vote_layout(nullptr, -1, 5, &wv));
  ParseGraphWs wgr;
  CHECK(!parse_graph_layout(nullptr, -1, 1, 1, &wgr) && !parse_graph_layout(nullptr, 1, -1, 1, &wgr) && !parse_graph_layout(nullptr, 1, 1, -1, &wgr));
  ParseVisWs wvi;
  CHECK(!parse_vis_layout(nullptr, -1, 1, &wvi) && !parse_vis_layout(nullptr, 1, -1, &wvi));
  MeshWs wm;
  CHECK(!mesh_layout(nullptr, 1, 2, 2, MESH_TILE, &wm) && !mesh_layout(nullptr, 2, 1, 2, MESH_TILE, &wm) && !mesh_layout(nullptr, 2, 2, 1, MESH_TILE, &wm));
  CHECK(!mesh_layout(nullptr, 2048, 2048, 512, MESH_TILE, &wm) && !mesh_layout(nullptr, 65536, 65536, 2, MESH_TILE, &wm) &&
        !mesh_layout(nullptr, 0, 4, 4, MESH_TILE, &wm));
  SumTreeWs wt;
  CHECK(!sum_tree_layout(nullptr, -1, FRAME_WG, FRAME_WG, 1, &wt));
  EvalGridWs we;
  CHECK(!eval_grid_layout(nullptr, -1, 1, &we) && !eval_grid_layout(nullptr, 1, 0, &we));
  EvalTriWs wet;
  CHECK(!eval_tri_layout(nullptr, -1, &wet));
  ShowWs wsh;
  CHECK(!show_layout(nullptr, 0, 1, 1, SHOW_QUEUE_CAP, &wsh) && !show_layout(nullptr, 1, 0, 1, SHOW_QUEUE_CAP, &wsh) &&
        !show_layout(nullptr, 1, 1, 0, SHOW_QUEUE_CAP, &wsh) && !show_layout(nullptr, 1, 32769, 1, SHOW_QUEUE_CAP, &wsh) &&
        !show_layout(nullptr, 1, 1, 32769, SHOW_QUEUE_CAP, &wsh) && !show_layout(nullptr, 2048, 32768, 32768, SHOW_QUEUE_CAP, &wsh));
  TraceWs wtr;
  CHECK(!trace_layout(nullptr, 0, TRACE_WG, &wtr) && !trace_layout(nullptr, -1, TRACE_WG, &wtr) && !trace_layout(nullptr, TRACE_MAX_RAYS + 1, TRACE_WG, &wtr));
  RaycastWs wrc;
  CHECK(!raycast_layout(nullptr, nullptr, -1, RC_WG, RC_TRI_STRIDE, &wrc) && !raycast_layout(nullptr, nullptr, RC_MAX_FACES + 1, RC_WG, RC_TRI_STRIDE, &wrc));
  DetectWs wd;
  CHECK(!detect_layout(nullptr, -1, 16, 16, 1.0, 5, DET_TILE, DET_WG, &wd) && !detect_layout(nullptr, 1, 1, 16, 1.0, 5, DET_TILE, DET_WG, &wd) &&
        !detect_layout(nullptr, 1, 16, 1, 1.0, 5, DET_TILE, DET_WG, &wd) && !detect_layout(nullptr, 1, 16, 16, 0.0, 5, DET_TILE, DET_WG, &wd) &&
        !detect_layout(nullptr, 1, 16, 16, 1.5, 5, DET_TILE, DET_WG, &wd) && !detect_layout(nullptr, 1, 16, 16, 1.0, 0, DET_TILE, DET_WG, &wd) &&
        !detect_layout(nullptr, 1, 32769, 16, 1.0, 5, DET_TILE, DET_WG, &wd) && !detect_layout(nullptr, 4096, 32768, 32768, 1.0, 5, DET_TILE, DET_WG, &wd));
  CHECK(detect_maps_ok(3, 129, 129, DET_TILE) && !detect_maps_ok(-1, 4, 4, DET_TILE) && !detect_maps_ok(3, 65536, 65536, DET_TILE) &&
        !detect_maps_ok(70000, 32768, 1, DET_TILE));
  TriWs wtri;
  CHECK(!tri_layout(nullptr, -1, 0, 0, 0, TRI_WG, &wtri) && !tri_layout(nullptr, 2, -1, 1, 0, TRI_WG, &wtri) &&
        !tri_layout(nullptr, 2, 4, -1, 4, TRI_WG, &wtri) && !tri_layout(nullptr, 2, 4, 1, -1, TRI_WG, &wtri) &&
        !tri_layout(nullptr, 2, 4, 2, 4, TRI_WG, &wtri) && !tri_layout(nullptr, 2, 4, 1, 5, TRI_WG, &wtri) &&
        !tri_layout(nullptr, TRI_MAX_VIEWS + 1, 4, 1, 4, TRI_WG, &wtri) && !tri_layout(nullptr, 2, 0x7fffffff / 10 + 1, 1, 10, TRI_WG, &wtri) &&
        !tri_layout(nullptr, 20, 1 << 27, 17, 10, TRI_WG, &wtri) && !tri_layout(nullptr, TRI_MAX_VIEWS, 1 << 24, 64, 1 << 24, TRI_WG, &wtri));
  Wf2dWs wwf;
  CHECK(!wf2d_layout(nullptr, -1, 0, 0, WF_WG, &wwf) && !wf2d_layout(nullptr, 1, -1, 0, WF_WG, &wwf) && !wf2d_layout(nullptr, 1, 4, -1, WF_WG, &wwf) &&
        !wf2d_layout(nullptr, 1, 4, 5, WF_WG, &wwf) && !wf2d_layout(nullptr, 0, 4, 4, WF_WG, &wwf) && !wf2d_layout(nullptr, 1, 4, 0, WF_WG, &wwf) &&
        !wf2d_layout(nullptr, WF_MAX_VIEWS + 1, 4, 4, WF_WG, &wwf) && !wf2d_layout(nullptr, 1, 0x7fffffff / 10 + 1, 1, WF_WG, &wwf) &&
        !wf2d_layout(nullptr, WF_MAX_VIEWS, 0x7fffffff / 10, 0x7fffffff / 10, WF_WG, &wwf));
  ScenegenWs wsg;
  CHECK(!scenegen_layout(nullptr, -1, 1, &wsg) && !scenegen_layout(nullptr, 1, -1, &wsg) && !scenegen_layout(nullptr, SG_MAX_VIEWS + 1, 1, &wsg) &&
        !scenegen_layout(nullptr, 1, 0x7fffffff / 8 + 1, &wsg) && !scenegen_layout(nullptr, 1000, 0x7fffffff / 4000 + 1, &wsg));
  CHECK(!scenegen_picture_ok(-1, 8, 8) && !scenegen_picture_ok(1, 0, 8) && !scenegen_picture_ok(1, 8, 0) && !scenegen_picture_ok(1, 32769, 8) &&
        !scenegen_picture_ok(1, 8, 32769) && !scenegen_picture_ok(SG_MAX_VIEWS + 1, 8, 8) && !scenegen_picture_ok(1000, 32768, 32768));
  // the two fixed blocks of partial results
  double* pd;
  float* pf;
  CHECK(partials_layout(nullptr, BOUNDS_BLOCKS, 6, &pd) == (size_t)BOUNDS_BLOCKS * 48 && ws_offset(nullptr, pd) == 0);
  CHECK(partials_layout(nullptr, FRAME_RANGE_BLOCKS, 2, &pf) == (size_t)FRAME_RANGE_BLOCKS * 8 && ws_offset(nullptr, pf) == 0);
  std::printf("ws_host_check: ok\n");
  return 0;
}
