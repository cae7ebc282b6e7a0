// Host-only check of the fragment-major index maps of the fp32 dgrad weight copies (net.h
// w2t_index / w3t_index): each is a bijection onto the copy, and a position decoded as
// [wave][instruction][lane][q] holds the weight element the loaders' comments promise
// (lnc3.h role 1: wa[tap][ko]; conv1.h c12_load_w2: wb[t][ks][ct]).
#include <cstdio>
#include <vector>

#include "../impala_amd/csrc/net.h"

using namespace net;

static int fails = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c) && ++fails <= 10) printf("FAIL line %d: %s\n", __LINE__, #c); \
  } while (0)

int main() {
  // ---- w3t: [ci tile ct = wave][tap * 4 + ko][lane][q], 36 instructions of 1 KB per wave ----
  {
    constexpr int N = OC3 * K3;  // 36864
    std::vector<int> hit(N, 0);
    for (int oc = 0; oc < OC3; ++oc)
      for (int tap = 0; tap < KS3 * KS3; ++tap)
        for (int ci = 0; ci < OC2; ++ci) {
          const int p = w3t_index(oc, tap, ci);
          CHECK(p >= 0 && p < N);
          if (p >= 0 && p < N) ++hit[p];
        }
    for (int p = 0; p < N; ++p) CHECK(hit[p] == 1);
    // the loader: wave ct, instruction i = tap * 4 + ko, lane l reads floats 4 l .. 4 l + 3 of the
    // instruction's 256 and must receive W3[oc = 16 ko + 4 (l >> 4) + q][tap][ci = 16 ct + (l & 15)]
    for (int ct = 0; ct < 4; ++ct)
      for (int i = 0; i < 36; ++i)
        for (int l = 0; l < 64; ++l)
          for (int q = 0; q < 4; ++q) {
            const int pos = ((ct * 36 + i) * 64 + l) * 4 + q;
            const int tap = i >> 2, ko = i & 3;
            CHECK(w3t_index(16 * ko + 4 * (l >> 4) + q, tap, 16 * ct + (l & 15)) == pos);
          }
  }
  // ---- w2t: [class cls = wave][(t * 4 + ks) * 2 + ct][lane][q], 32 instructions per wave, a
  // tap t of the class 8 KB contiguous ----
  {
    constexpr int N = OC2 * K2;  // 32768
    std::vector<int> hit(N, 0);
    for (int oc = 0; oc < OC2; ++oc)
      for (int kh = 0; kh < KS2; ++kh)
        for (int kw = 0; kw < KS2; ++kw)
          for (int ci = 0; ci < OC1; ++ci) {
            const int p = w2t_index(oc, kh, kw, ci);
            CHECK(p >= 0 && p < N);
            if (p >= 0 && p < N) ++hit[p];
          }
    for (int p = 0; p < N; ++p) CHECK(hit[p] == 1);
    // the loader: wave cls = (py, px), tap t -> (kh, kw) = (py + 2 (t >> 1), px + 2 (t & 1)),
    // instruction (t * 4 + ks) * 2 + ct, lane l must receive
    // W2[oc = 16 ks + 4 (l >> 4) + q][kh][kw][ci = 16 ct + (l & 15)]
    for (int cls = 0; cls < 4; ++cls)
      for (int i = 0; i < 32; ++i)
        for (int l = 0; l < 64; ++l)
          for (int q = 0; q < 4; ++q) {
            const int pos = ((cls * 32 + i) * 64 + l) * 4 + q;
            const int t = i >> 3, ks = (i >> 1) & 3, ct = i & 1;
            const int kh = (cls >> 1) + 2 * (t >> 1), kw = (cls & 1) + 2 * (t & 1);
            CHECK(w2t_index(16 * ks + 4 * (l >> 4) + q, kh, kw, 16 * ct + (l & 15)) == pos);
            CHECK(pos / 2048 == cls * 4 + t);  // the tap's own 8 KB
          }
  }
  // the copies keep their sizes in the shadow buffer
  const Shadow sh = shadow();
  CHECK(sh.w3t - sh.w2t == (size_t)OC2 * K2 && sh.total - sh.w3t == (size_t)OC3 * K3);
  if (fails) {
    printf("wfrag: %d checks failed\n", fails);
    return 1;
  }
  printf("wfrag ok\n");
  return 0;
}
