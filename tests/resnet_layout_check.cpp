// CPU check of impala_amd/csrc/resnet_layout.h (tests/test_resnet_layout.py).  Prints flat_offsets(A)
// in state_dict order and the total for A = 1, 6, 15 (the test holds them to param_specs), then runs
// the handle's two-pass carve over four configurations: the sizing pass and the real pass agree, every
// buffer is 256-byte aligned and inside the block, no two overlap given the sizes spelled out here,
// and the buffers a configuration does not have are null.
#include "../impala_amd/csrc/arena.h"
#include "../impala_amd/csrc/resnet_layout.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                    \
    }                                                              \
  } while (0)

static int check_carve(int batch, int dtype, int debug, int train, int n_cu, int want_groups) {
  const resnet_config cfg{batch, 15, dtype, debug, train};
  ResnetBufs b;
  const size_t total = resnet_carve(b, cfg, n_cu, Arena{});
  CHECK(total > 0 && total % 256 == 0);
  CHECK(!b.w[0] && !b.wfc && !b.vecs && !b.y && !b.part && !b.h && !b.heads && !b.stages && !b.slab);  // sizing: all null
  char* block = (char*)std::aligned_alloc(256, total);  // (never touched)
  CHECK(block);
  Arena real{block};
  CHECK(resnet_carve(b, cfg, n_cu, real) == total);

  CHECK(resnet_wg_groups(batch, n_cu) == want_groups);
  const size_t es = dtype == IMPALA_DTYPE_BF16 ? 2 : 4, B = (size_t)batch, ks = es == 2 ? 32 : 16;
  std::vector<std::pair<const void*, size_t>> bufs;  // (pointer, bytes) of every buffer the configuration has
  for (int id = 0; id < RN_CONVS; ++id) {
    const size_t k = 9 * (size_t)(id == 0 ? 4 : conv_geo(id).cin);  // the stem's pixels are 4 wide
    bufs.push_back({b.w[id], conv_geo(id).cout * ((k + ks - 1) / ks * ks) * es});
  }
  bufs.push_back({b.wfc, (size_t)256 * 2048 * es});
  bufs.push_back({b.vecs, (size_t)(15 * 32 + 2 * 2048 + 256 + 16 * 256 + 16) * 4});
  bufs.push_back({b.y, B * 2048 * es});
  bufs.push_back({b.part, 8 * B * 256 * 4});
  bufs.push_back({b.h, B * 256 * es});
  bufs.push_back({b.heads, B * 16 * 4});
  const size_t frame = 5 * 32 * 32 * 16 + 5 * 16 * 16 * 32 + 5 * 8 * 8 * 32;
  CHECK(frame == (size_t)RN_DBG_FRAME && stage_at(batch, 14, batch - 1) + dbg_size(14) == B * frame);
  if (debug || train) bufs.push_back({b.stages, B * frame * es});
  else CHECK(!b.stages);
  if (train) {
    bufs.push_back({b.amax, B * (32 * 32 * 16 + 16 * 16 * 32 + 8 * 8 * 32)});  // a byte per pooled element
    bufs.push_back({b.lnstat, B * 2 * 4});
    CHECK(!b.wd[0]);  // the stem has no data gradient
    for (int id = 1; id < RN_CONVS; ++id) bufs.push_back({b.wd[id], (size_t)conv_geo(id).cout * conv_geo(id).cin * 9 * 4});
    bufs.push_back({b.wfct, (size_t)256 * 2048 * 4});
    bufs.push_back({b.gz, B * 256 * 4});
    bufs.push_back({b.gy, B * 2048 * 4});
    bufs.push_back({b.gws, B * frame * 4});
    bufs.push_back({b.slab, (size_t)want_groups * RESNET_BODY_PARAMS * 4});
  } else {
    CHECK(!b.amax && !b.lnstat && !b.wfct && !b.gz && !b.gy && !b.gws && !b.slab);
    for (int id = 0; id < RN_CONVS; ++id) CHECK(!b.wd[id]);
  }
  std::sort(bufs.begin(), bufs.end());
  const char* end = block;
  for (const auto& pb : bufs) {
    const char* p = (const char*)pb.first;
    CHECK(p != nullptr && pb.second > 0);
    CHECK((size_t)(p - block) % 256 == 0);
    CHECK(p >= end);  // past the buffer before it
    end = p + pb.second;
  }
  CHECK(end <= block + total);
  std::free(block);
  return 0;
}

int main() {
  for (int A : {1, 6, 15}) {
    const GradOff g = flat_offsets(A);
    std::printf("offsets %d", A);
    for (int id = 0; id < RN_CONVS; ++id) std::printf(" %d %d", g.w[id], g.b[id]);
    std::printf(" %d %d %d %d %d %d %d %d total %zu\n", g.lng, g.lnb, g.wfc, g.bfc, g.wa, g.ba, g.wc, g.bc, flat_total(A));
  }
  //              batch dtype              debug train n_cu groups
  if (check_carve(1, IMPALA_DTYPE_F32, 0, 0, 256, 1)) return 1;
  if (check_carve(17, IMPALA_DTYPE_BF16, 1, 0, 256, 17)) return 1;
  if (check_carve(17, IMPALA_DTYPE_F32, 0, 1, 3, 1)) return 1;
  if (check_carve(160, IMPALA_DTYPE_F32, 1, 1, 256, 64)) return 1;
  std::printf("carve ok\n");
  return 0;
}
