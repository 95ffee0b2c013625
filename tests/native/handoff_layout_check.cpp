// Host check of handoff_layout.h (the blocked hand-off layout of the fused LeNet step) for the LeNet
// shapes: the weight-gradient tile's operand delivery against the plain [F][M] addressing, the
// LDS-DMA image against the fragment reads, and a bank model of the ds_read_b64 lane groups.
// Exit status 0 = all checks passed; every failure prints one line.
#include "handoff_layout.h"

#include <cstdio>
#include <vector>

namespace ho = rk_handoff;

static int g_fail = 0;
#define CHECK(c, ...)                     \
  do {                                    \
    if (!(c)) {                           \
      if (++g_fail <= 20) {               \
        std::printf("FAIL %s: ", #c);     \
        std::printf(__VA_ARGS__);         \
        std::printf("\n");                \
      }                                   \
    }                                     \
  } while (0)

// an element's identity: (feature, sample); pads are -1
static int code(int f, int n, int M) { return f * M + n; }

struct Tensor {
  int F, Fp, M;
  std::vector<int> plain;    // [F][M]
  std::vector<int> blocked;  // [M / 4][Fp][4]
  Tensor(int F_, int M_) : F(F_), Fp(ho::padded(F_)), M(M_), plain((size_t)F_ * M_), blocked((size_t)M_ / 4 * ho::padded(F_) * 4, -1) {
    for (int f = 0; f < F; ++f)
      for (int n = 0; n < M; ++n) {
        plain[(size_t)f * M + n] = code(f, n, M);
        blocked[(size_t)ho::offset(Fp, n / 4, f) + n % 4] = code(f, n, M);
      }
  }
};

// what the plain addressing hands lane (feature r, samples m0 .. m0 + 7): zeros (here -2) out of range
static void plain_frag(const Tensor& T, int r, int m0, int out[8]) {
  const bool ok = r < T.F && m0 < T.M;
  for (int e = 0; e < 8; ++e) out[e] = ok ? T.plain[(size_t)r * T.M + m0 + e] : -2;
}

// ---- global-load path: two 8-byte loads per fragment
static void check_global(int F, int M, int tile, int width) {
  const Tensor T(F, M);
  const int per = ((M + 8 * 64 - 1) / (8 * 64)) * 64;
  for (int wv = 0; wv < 8; ++wv) {
    const int mb = wv * per, me = M < mb + per ? M : mb + per;
    for (int m = mb; m < me; m += 128)
      for (int s = 0; s < 4; ++s)
        for (int hi = 0; hi < 4; ++hi)
          for (int f0 = 0; f0 < (F + tile - 1) / tile * tile; f0 += tile)
            for (int lf = 0; lf < width; ++lf) {
              const int mk = m + 32 * s + 8 * hi, mm = mk < me ? mk : M, r = f0 + lf;
              int want[8], got[8];
              plain_frag(T, r, mm, want);
              const bool ok = r < F && mm < M;
              for (int h = 0; h < 2; ++h) {
                const int64_t o = ho::frag_offset(T.Fp, ok ? mm : 0, h, r < F ? r : 0);
                CHECK(o >= 0 && o + 4 <= (int64_t)T.blocked.size(), "global load out of bounds F=%d M=%d", F, M);
                for (int j = 0; j < 4; ++j) got[4 * h + j] = ok ? T.blocked[(size_t)o + j] : -2;
              }
              for (int e = 0; e < 8; ++e)
                CHECK(got[e] == want[e], "global path F=%d M=%d r=%d m=%d e=%d: %d != %d", F, M, r, mm, e, got[e], want[e]);
            }
  }
}

// ---- LDS-DMA path (M = 1024): one wave's staged image of a (d tile, x tile) pair
static void check_lds(int N, int K, int M) {
  const Tensor D(N, M), X(K, M);
  const int units = (ho::kDBytes + ho::kWaveRecords * ho::kXTile * 8) / 2;  // 16-bit elements per wave
  for (int n0 = 0; n0 < N; n0 += ho::kDTile)
    for (int k0 = 0; k0 < K; k0 += ho::kXTile)
      for (int wv = 0; wv < 8; ++wv) {
        const int mb = wv * 128, rec0 = mb / 4;
        std::vector<int> lds(units, -3), writes(units / 8, 0);
        // the image: piece q, lane -> 16 bytes (8 elements) at q * 1024 + lane * 16
        std::vector<int> fetched_d(ho::kWaveRecords * ho::kDTile / 2, 0), fetched_x(ho::kWaveRecords * ho::kXTile / 2, 0);
        for (int q = 0; q < ho::kDPieces + ho::kXPieces; ++q)
          for (int lane = 0; lane < 64; ++lane) {
            const bool isd = q < ho::kDPieces;
            const Tensor& T = isd ? D : X;
            const int qq = isd ? q : q - ho::kDPieces;
            const int rec = isd ? ho::dma_d_rec(qq, lane) : ho::dma_x_rec(qq, lane);
            const int tf = isd ? ho::dma_d_feat(lane) : ho::dma_x_feat(qq, lane);
            const int f = isd ? n0 + tf : ho::clamp_feat(k0 + tf, T.Fp);
            CHECK(rec >= 0 && rec < ho::kWaveRecords && tf >= 0 && tf + 2 <= (isd ? ho::kDTile : ho::kXTile), "chunk range");
            CHECK(f >= 0 && f + 2 <= T.Fp, "source chunk leaves the record: f=%d Fp=%d", f, T.Fp);
            (isd ? fetched_d : fetched_x)[rec * (isd ? ho::kDTile : ho::kXTile) / 2 + tf / 2]++;
            const int64_t o = ho::offset(T.Fp, rec0 + rec, f);
            CHECK(o % 8 == 0 && o + 8 <= (int64_t)T.blocked.size(), "DMA source unaligned or out of bounds");
            const int dst = (q * 1024 + lane * 16) / 2;
            writes[dst / 8]++;
            for (int j = 0; j < 8; ++j) lds[dst + j] = T.blocked[(size_t)o + j];
          }
        for (int c : fetched_d) CHECK(c == 1, "a d chunk fetched %d times", c);
        for (int c : fetched_x) CHECK(c == 1, "an x chunk fetched %d times", c);
        for (int c : writes) CHECK(c == 1, "an LDS chunk written %d times", c);
        // the fragment reads: every 8-byte unit of the image is read by exactly one (s, hi, h, feature)
        std::vector<int> reads(units / 4, 0);
        for (int s = 0; s < 4; ++s)
          for (int hi = 0; hi < 4; ++hi)
            for (int op = 0; op < 3; ++op)  // d, x (j = 0), x (j = 1)
              for (int lo = 0; lo < 16; ++lo) {
                const bool isd = op == 0;
                const Tensor& T = isd ? D : X;
                const int tf = isd ? lo : 16 * (op - 1) + lo, r = (isd ? n0 : k0) + tf;
                int want[8];
                plain_frag(T, r, mb + 32 * s + 8 * hi, want);
                for (int h = 0; h < 2; ++h) {
                  const int a = isd ? ho::lds_d(s, hi, h, tf) : ho::kDBytes + ho::lds_x(s, hi, h, tf);
                  CHECK(a % 8 == 0 && a >= (isd ? 0 : ho::kDBytes) && a + 8 <= (isd ? ho::kDBytes : units * 2), "fragment read range");
                  reads[a / 8]++;
                  for (int j = 0; j < 4; ++j) {
                    const int got = lds[a / 2 + j];
                    // live features: exactly the plain addressing's element, so never a pad; features
                    // past the tensor (outputs not stored) may hold a pad or the tile's clamped half
                    if (r < T.F) CHECK(got == want[4 * h + j], "lds path N=%d K=%d op=%d r=%d s=%d hi=%d e=%d: %d != %d", N, K, op, r, s, hi, 4 * h + j, got, want[4 * h + j]);
                    else CHECK(got == -1 || (got >= 0 && got / M >= k0 && got / M < T.F), "dead feature read %d", got);
                  }
                }
              }
        for (int c : reads) CHECK(c == 1, "an LDS 8-byte unit read %d times", c);
        if (g_fail) return;
      }
}

// ---- ds_read_b64 bank model: lane groups {0-31}, {32-63}; bank of byte a = (a / 4) mod 64; each
// extra distinct address on a bank is one more cycle
static void check_banks() {
  int worst = 0;
  for (int s = 0; s < 4; ++s)
    for (int h = 0; h < 2; ++h)
      for (int op = 0; op < 3; ++op)
        for (int g = 0; g < 2; ++g) {
          int cnt[64] = {0};
          for (int l = 0; l < 32; ++l) {
            const int lane = 32 * g + l, lo = lane & 15, hi = lane >> 4;
            const int a = op == 0 ? ho::lds_d(s, hi, h, lo) : ho::kDBytes + ho::lds_x(s, hi, h, 16 * (op - 1) + lo);
            cnt[(a / 4) % 64]++;
            cnt[(a / 4 + 1) % 64]++;
          }
          for (int b = 0; b < 64; ++b) worst = cnt[b] > worst ? cnt[b] : worst;
        }
  std::printf("ds_read_b64 conflict degree: %d (stated: %d)\n", worst, ho::kConflictDegree);
  CHECK(worst <= ho::kConflictDegree, "bank conflict degree %d", worst);
  // the merged form (ds_read2_b64 / ds_read2st64_b64, two of the reads above in one instruction): each
  // access is served in four groups of 16 contiguous lanes; bank of byte a = (a / 4) mod 32
  int worst2 = 0;
  for (int s = 0; s < 4; ++s)
    for (int h = 0; h < 2; ++h)
      for (int op = 0; op < 3; ++op)
        for (int g = 0; g < 4; ++g) {
          int cnt[32] = {0};
          for (int l = 0; l < 16; ++l) {
            const int lane = 16 * g + l, lo = lane & 15, hi = lane >> 4;
            const int a = op == 0 ? ho::lds_d(s, hi, h, lo) : ho::kDBytes + ho::lds_x(s, hi, h, 16 * (op - 1) + lo);
            cnt[(a / 4) % 32]++;
            cnt[(a / 4 + 1) % 32]++;
          }
          for (int b = 0; b < 32; ++b) worst2 = cnt[b] > worst2 ? cnt[b] : worst2;
        }
  std::printf("ds_read2_b64 conflict degree: %d (stated: %d)\n", worst2, ho::kConflictDegree);
  CHECK(worst2 <= ho::kConflictDegree, "bank conflict degree %d (ds_read2_b64 form)", worst2);
}

int main() {
  static_assert(ho::padded(400) == 400 && ho::padded(120) == 128 && ho::padded(84) == 96 && ho::padded(10) == 16, "Fp");
  const int shapes[3][2] = {{10, 84}, {84, 120}, {120, 400}};  // (N, K) of fc3, fc2, fc1
  for (const auto& sh : shapes) {
    check_lds(sh[0], sh[1], 1024);
    for (int M : {8, 40, 520, 1024}) {
      check_global(sh[0], M, 16, 16);
      check_global(sh[1], M, 32, 32);
    }
  }
  check_banks();
  std::printf(g_fail ? "handoff layout: %d FAILURES\n" : "handoff layout: ok\n", g_fail);
  return g_fail ? 1 : 0;
}
