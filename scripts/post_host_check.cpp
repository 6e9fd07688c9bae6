// Stand-alone check of the host-side helpers of neat_amd/csrc/kernels_post.hpp (count bounds, workspace offsets) under the
// host sanitizers.  No device is touched.  Build and run (host code only is instrumented):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Ineat_amd/csrc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         scripts/post_host_check.cpp -o /tmp/post_host_check && /tmp/post_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels_post.hpp"

using namespace neat;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// every region of a layout is 256-byte aligned, in order, disjoint, and holds what the kernels index
static bool ordered(const std::vector<size_t>& offs, const std::vector<size_t>& need, size_t total) {
  for (size_t i = 0; i < offs.size(); ++i) {
    if (offs[i] % 256 != 0) return false;
    const size_t end = i + 1 < offs.size() ? offs[i + 1] : total;
    if (end < offs[i] || end - offs[i] < need[i]) return false;
  }
  return true;
}

int main() {
  // count bounds
  CHECK(post_counts_ok(0, 0, 0) && post_counts_ok(50000, 64, 32000) && post_counts_ok(0x7fffffffLL / 6, 1, 0));
  CHECK(!post_counts_ok(-1, 1, 1) && !post_counts_ok(1, -1, 1) && !post_counts_ok(1, 1, -1));
  CHECK(!post_counts_ok(0x7fffffffLL / 6 + 1, 1, 0) && !post_counts_ok(10, POST_MAX_VIEWS + 1, 0));
  CHECK(!post_counts_ok(0x7fffffffLL / 6, 7, 0));                          // n V beyond an int
  CHECK(post_grid_ok(2) && post_grid_ok(512) && post_grid_ok(1024) && !post_grid_ok(1) && !post_grid_ok(1025) && !post_grid_ok(2048) &&
        !post_grid_ok(-4));
  CHECK((long long)(POST_MAX_GRID - 1) * POST_MAX_GRID * POST_MAX_GRID + (long long)(POST_MAX_GRID - 1) * POST_MAX_GRID + POST_MAX_GRID - 1 <
        (1LL << 30));                                                       // the largest cell key
  // layouts
  for (long long n : {0LL, 1LL, 255LL, 256LL, 257LL, 50000LL}) {
    for (long long V : {0LL, 1LL, 3LL, 64LL}) {
      for (long long mt : {0LL, 1LL, 1025LL, 32000LL}) {
        PostFuseWs w;
        CHECK(post_fuse_layout(n, V, mt, &w));
        CHECK(ordered({w.label, w.present, w.rank, w.idx}, {(size_t)(n * V * 4), (size_t)mt, (size_t)(mt * 4), (size_t)(n * 4)}, w.total));
      }
    }
    for (long long mm : {0LL, 1LL, 500LL}) {
      PostRefineWs w;
      CHECK(post_refine_layout(n, mm, 12345, &w));
      CHECK(ordered({w.label, w.idx, w.glines, w.gscores, w.gcount, w.group},
                    {(size_t)(8 * n), (size_t)(4 * n), (size_t)(24 * mm), (size_t)(4 * mm), sizeof(int), (size_t)12345}, w.total));
    }
    for (long long G : {2LL, 8LL, 512LL, 1024LL}) {
      PostSnapWs w;
      CHECK(post_snap_layout(n, G, 777, &w));
      const size_t M4 = (size_t)(8 * n);
      CHECK(ordered({w.box, w.counts, w.key, w.skey, w.head, w.flag, w.cnt, w.pidx, w.near, w.dist2, w.idx, w.pkey, w.spkey, w.sort},
                    {36, 8, M4, M4, M4, M4, M4, M4, M4, M4, (size_t)(4 * n), (size_t)(8 * n), (size_t)(8 * n), 777}, w.total));
    }
    PostSnapWs w;
    CHECK(!post_snap_layout(n, 2048, 0, &w) && !post_snap_layout(n, 1, 0, &w));
  }
  PostFuseWs wf;
  CHECK(!post_fuse_layout(0x7fffffffLL, 1, 0, &wf) && !post_fuse_layout(10, 70000, 0, &wf));
  std::printf("post_host_check: ok\n");
  return 0;
}
