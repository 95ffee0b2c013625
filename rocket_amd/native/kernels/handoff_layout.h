// Blocked hand-off layout of the fused LeNet step: the six 16-bit tensors the step kernel hands to
// the grouped weight-gradient launch (a2, h1, h2 and the gradients d1, d2, dy).
//
// A tensor of F features over N samples is [N / 4][Fp][4]: one RECORD per group of 4 samples (the
// step kernel's block), Fp = F padded to a multiple of 16, so a record is a whole number of 128-byte
// lines and a block writes only lines it owns.  A feature's 4 samples are one 8-byte value.
// Pad features (f >= F) may hold anything; no reader lets them reach a gradient.
//
// The weight-gradient tile (16 d features x 32 x features, a wave's 128 samples = 32 records) stages
// its operands by LDS-DMA: a 1-KiB piece is 64 lanes x 16 bytes, written lane-linear, so a piece holds
// 8 records x 128 B of d or 4 records x 256 B of x.  The MFMA fragment of lane (lo, hi) at k-step s
// (samples 32 s + 8 hi .. + 7 of feature lo) is two 8-byte LDS reads, half h from record
// 8 s + 2 hi + h.  The functions below are the whole index math; they are constexpr and also compile
// on the host, where tests/unit checks them.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RK_HD __host__ __device__
#else
#define RK_HD
#endif

namespace rk_handoff {

constexpr int kSamples = 4;        // samples per record
constexpr int kWaveRecords = 32;   // records of a wave's 128-sample batch range
constexpr int kDTile = 16, kXTile = 32;  // features of a weight-gradient tile's two operands
constexpr int kDPieces = 4, kXPieces = 8;  // 1-KiB DMA pieces per wave
constexpr int kDBytes = kWaveRecords * kDTile * 8;  // staged d operand (4 KiB); x follows it (8 KiB)

RK_HD constexpr int padded(int F) { return (F + 15) & ~15; }

// element offset (16-bit units) of feature f's 4-sample value in record rec
RK_HD constexpr int64_t offset(int Fp, int64_t rec, int f) { return (rec * Fp + f) * kSamples; }
// fragment-shaped global loads: half h (samples m0 + 4 h .. + 3, m0 % 8 == 0) of feature f
RK_HD constexpr int64_t frag_offset(int Fp, int m0, int h, int f) { return offset(Fp, m0 / kSamples + h, f); }

// Bank swizzle.  A ds_read_b64 is served in two groups of 32 lanes (hi in {0, 1} and {2, 3}) over
// 64 banks of 4 bytes; a group reads 16 features (128 B) of two records that lie 2 records apart,
// which unswizzled are 256 B (d) or 512 B (x) apart: the same banks, a 2-way conflict.  Bit 1 of the
// record number therefore flips which 128-byte half of a 256-byte bank window a record's features
// take: the neighbouring record's slot for d, the other half of the record for x.  With it every
// lane group touches each bank exactly once: conflict degree 1 (checked by the host test's model).
// The compiler merges most of these reads, pairwise over consecutive k-steps (1 or 2 KiB apart), into
// ds_read2st64_b64.  Each of that instruction's two accesses is served in four groups of 16
// contiguous lanes over 32 banks (at half the bytes per clock); such a group is the 16 features of one
// record, 128 contiguous bytes = each of the 32 banks once, with or without the swizzle.  So the
// degree is 1 under either form; the host test models both.
constexpr int kConflictDegree = 1;
RK_HD constexpr int bit1(int rec) { return (rec >> 1) & 1; }
RK_HD constexpr int d_slot(int rec) { return rec ^ bit1(rec); }  // an involution

// ---- LDS-DMA image: which source chunk lane `lane` of piece q fetches (record within the wave's
// range, first feature of its 16-byte = 2-feature chunk relative to the tile's first feature)
RK_HD constexpr int dma_d_rec(int q, int lane) { return d_slot(8 * q + (lane >> 3)); }
RK_HD constexpr int dma_d_feat(int lane) { return 2 * (lane & 7); }
RK_HD constexpr int dma_x_rec(int q, int lane) { return 4 * q + (lane >> 4); }
RK_HD constexpr int dma_x_feat(int q, int lane) { return 2 * ((lane & 15) ^ (8 * bit1(dma_x_rec(q, lane)))); }
// An x tile may reach past the padded record (400 features: the last tile holds 16).  Such chunks
// fetch the tile's live half instead; they feed output columns >= K only, which are never stored.
RK_HD constexpr int clamp_feat(int f, int Fp) { return f < Fp ? f : f - 16; }

// ---- fragment reads: byte address, within the wave's staged d (resp. x) operand, of half h of the
// fragment of tile feature f (d: lo; x: 16 j + lo) for lane row hi at k-step s
RK_HD constexpr int frag_rec(int s, int hi, int h) { return 8 * s + 2 * hi + h; }
RK_HD constexpr int lds_d(int s, int hi, int h, int f) { return d_slot(frag_rec(s, hi, h)) * 128 + f * 8; }
RK_HD constexpr int lds_x(int s, int hi, int h, int f) {
  return frag_rec(s, hi, h) * 256 + (((f >> 1) ^ (8 * bit1(frag_rec(s, hi, h)))) * 16) + (f & 1) * 8;
}

}  // namespace rk_handoff
