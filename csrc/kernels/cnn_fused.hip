// Fused MNIST-CNN training step for gfx950: the whole of horovod/mnist_horovod.py:9-25's `Net`
// (conv5x5 1->10, maxpool2, ReLU, conv5x5 10->20, Dropout2d, maxpool2, ReLU, fc 320->50, ReLU,
// dropout, fc 50->10, log_softmax) + NLL loss + the complete backward pass, with every activation
// resident in LDS.
//
// Why: the network is 21,840 parameters and ~1 MFLOP/image forward; at the reference batch (1024 per
// worker) the layer-by-layer path is ~40 kernels of a few microseconds each, every one far below the
// chip's roofline.  Here ONE workgroup (16 wave64s, one per CU: the LDS image is
// ~122 KB) trains NI=4 images end to end.  Every phase is a short dependent chain (LDS gathers feeding a
// few MFMAs, L2 weight loads feeding a dot product), so the kernel is latency-bound: 16 waves (4 per
// SIMD, <= 128 VGPRs) hide twice the latency of 8 and cut each phase's per-wave trip count in half:
//   * the five convolution GEMMs -- conv1 fwd, conv2 fwd, conv2 dgrad, conv2 wgrad, conv1 wgrad -- run
//     on the matrix cores (v_mfma_f32_16x16x32_bf16, fp32 accumulate) as implicit GEMMs whose operand
//     fragments are gathered straight from the LDS-resident bf16 activations (im2col never exists);
//   * the conv weights are re-laid out ONCE per workgroup into LDS in MFMA B-fragment order (one 16-byte
//     ds_read per lane per fragment); fc1's 64 KB weight matrix is read from L2 (shared by all WGs);
//   * the forward M dimension is ordered (pooled cell, 2x2 tap), so an MFMA lane's 4 accumulator rows
//     are exactly the 4 taps of one pooling window: max-pool, argmax, bias, dropout2d and ReLU are done
//     on the accumulators, and no pre-pool activation is ever stored;
//   * backward scatters the pooled gradients to their argmax taps once (a dense bf16 plane per channel)
//     and feeds it to the dgrad / wgrad GEMMs; small fc layers, softmax/NLL and masks stay in fp32 VALU;
//   * every weight gradient of the 4 images is complete after its phase and is written straight to the
//     workgroup's fp32 slab; k_cnn_reduce sums the slabs in a fixed order (deterministic) straight into
//     the flat gradient buffer (e.g. the DDP bucket).
// Dropout masks come from a counter-based hash keyed by a device-resident counter that k_cnn_reduce
// advances, so hipGraph replays draw fresh masks.  Precision: bf16 MFMA operands (images, conv weights,
// conv activations and their gradients), fp32 accumulation, fp32 fc layers / loss / gradients.
#include <cstddef>
#include <type_traits>

#include "adasum_weights.h"
#include "common.cuh"
#include "optim_device.h"
#include "pde_kernels.h"
#include "xgmi_device.h"

namespace pde {

namespace {

constexpr int T = 1024;           // 16 waves
constexpr int NW = T / 64;
constexpr int NI = 4;             // images per workgroup
constexpr int C1 = 10, C2 = 20, KS = 5, H0 = 28, O1 = 24, P1 = 12, O2 = 8, P2 = 4, F1 = 50, F2 = 10;
constexpr int NX = H0 * H0, NC1 = P1 * P1, NR1 = C1 * NC1, NC2 = P2 * P2, NIN = C2 * NC2;  // 784 144 1440 16 320
// LDS channel pitches of the [ci][cell] planes (r1 in u16, a1 in bytes, e1 in u32): 144 cells padded so that the
// channels a wave touches at once fall in different banks (ds_*_b32 banks are (a / 4) mod 32; at a 288-byte
// pitch channels 0, 4, 8 share one: P1's stores and P9's reads ran 3-6 LDS cycles per instruction, r4s)
constexpr int RP16 = 146, RP8 = 148;
static_assert(RP16 >= NC1 && RP8 >= NC1, "channel planes hold the 144 cells");
static_assert(RP16 % 2 == 0 && RP8 % 4 == 0, "P9 reads 4 cells' argmax bytes as one aligned 4-byte word");
// e1: the conv1-output gradient of every pooled cell, written by P7b's epilogue as a bf16 pair positioned at its
// argmax tap's column (tap dx = 0 -> low half, 1 -> high half; 0 for a relu-dead cell) and read by P9 as 4 cells
// per 16-byte load.  592-byte channel rows: 16-byte aligned, and the 10 channels of a 16-lane b128 phase start
// 20 banks apart (disjoint 4-bank spans)
constexpr int EP = 148;
constexpr unsigned char AM_DEAD = 0xFF;  // a1 of a relu-dead cell (r1 == 0): no tap carries a gradient
// LDS row pitch of the images x / x1 (28 pixels + 8 zero columns): with x1 9 banks after x, P1's pixel-pair
// gathers take 2.75 LDS cycles per instruction instead of 4 (r4t model; columns 28.. are read by the zero-weight
// kx = 5 taps only)
constexpr int XP = 36, NXP = H0 * XP;
constexpr int DHP = 52;  // LDS row pitch (floats) of dh: 16-byte rows, P6 reads them as float4
constexpr int W1N = C1 * KS * KS, W2N = C2 * C1 * KS * KS, FC1N = F1 * NIN, FC2N = F2 * F1;
constexpr int K2 = C1 * KS * KS;       // 250: conv2 reduction (ci,ky,kx) in the weight's own order
// conv2 fwd: K ordered (tap, ci) with ci padded to 16 over a channel-last copy of r1, so a lane's 8
// k-values are ONE 16-byte LDS read: k = 32 ks + 8 lg + j -> tap 2 ks + lg/2, ci 8 (lg & 1) + j
constexpr int C1P = 16;
constexpr int KS2 = (KS * KS * C1P + 31) / 32;  // 13 k-steps (the last one half padding)
constexpr int KSW2 = NI * 8 * 8 / 32;           // 8 conv2-wgrad k-steps: K = (image, y, x)
// conv2 dgrad: K = (tap, co) with co padded to 24 = 3 groups of 8, packed: k-step ks, lane group lg holds
// group g = 4 ks + lg = (tap g / 3, channels 8 (g % 3) .. +7).  The gradient is kept with each co group of 8
// contiguous (co 20..23 zero), so a lane's 8 k-values are ONE 16-byte LDS read of its own position.
constexpr int CG = 3;                                // co groups of 8 per tap
constexpr int NGD = KS * KS * CG;                    // 75 (tap, co-group) pairs
constexpr int KSD = (NGD + 3) / 4;                   // 19 k-steps (25 with one k-step per tap)
// d2n layout (u16 units): element (im, Y, X, co) at im D2N_IM + Y D2N_RP + X D2N_P + (co / 8) D2N_Q + co % 8 --
// 48-byte positions, 528-byte rows, co groups 256 bytes apart (interleaved with other positions' slots).  A P7b
// A read (a 16-lane b128 group mixes two k-groups and two rows of the tile) models 5.6 LDS cycles per
// wave-instruction against 6.75 for plain [pos][40] rows (scripts/p7b_lds_model.py; 4 is conflict-free)
constexpr int D2N_P = 24, D2N_RP = 264, D2N_Q = 128;
constexpr int D2N_IM = 7 * D2N_RP + 7 * D2N_P + 2 * D2N_Q + 8;  // 2280: one past the last slot of an image
static_assert(D2N_IM % 8 == 0 && D2N_P % 8 == 0 && D2N_RP % 8 == 0 && D2N_Q % 8 == 0, "d2n: 16-byte slots");
__host__ __device__ constexpr int d2n_ofs(int im, int y, int x, int co) {
  return im * D2N_IM + y * D2N_RP + x * D2N_P + (co >> 3) * D2N_Q + (co & 7);
}
constexpr int D2R = O2 * O2 + 8;       // d2 plane row stride (u16): 144 B
constexpr int MT1 = O1 * O1 / 16;      // 36 conv1 M-tiles per image (4 cells x 4 taps each)
constexpr int MTD = NC1 * 1 / 16;      // 9 conv2-dgrad M-tiles per image (144 r1 positions)
constexpr int KSW1 = O1 * O1 / 32;     // 18 conv1-wgrad k-steps per image
// conv2 dgrad k-step ranges.  A dgrad tile is 16 consecutive row-major positions of the 12x12 plane, so its class
// c = tile % MTD fixes the two rows Y it covers, and a source row Y - ky exists only for max(0, Y - 7) <= ky <=
// min(4, Y): with K ordered (ky, kx, co group) the k-steps in which ANY lane of the class reads a real source
// position are one contiguous run [lo, hi) of the KSD -- outside it every A fragment is the zero block and the
// MFMA adds exact zeros.  Derived from the geometry, per class; 126 of the 9 x 19 = 171 k-steps remain.
struct KsRange {
  int lo, hi;
};
__host__ __device__ constexpr bool p7b_tap_live(int cls, int r, int ky, int kx) {  // position r of the class, tap
  const int pos = cls * 16 + r, y = pos / P1 - ky, x = pos % P1 - kx;
  return y >= 0 && y < O2 && x >= 0 && x < O2;
}
__host__ __device__ constexpr KsRange p7b_ks_range(int cls) {
  int lo = KSD, hi = 0;
  for (int r = 0; r < 16; ++r)
    for (int ky = 0; ky < KS; ++ky)
      for (int kx = 0; kx < KS; ++kx) {
        if (!p7b_tap_live(cls, r, ky, kx)) continue;
        const int g0 = (ky * KS + kx) * CG, k0 = g0 / 4, k1 = (g0 + CG - 1) / 4;  // the tap's co groups' k-steps
        lo = k0 < lo ? k0 : lo;
        hi = k1 + 1 > hi ? k1 + 1 : hi;
      }
  return {lo, hi};
}
// every live (position, tap, co group) of the class lies inside [lo, hi) (checked group by group, not through
// the derivation's k0 / k1)
__host__ __device__ constexpr bool p7b_range_covers(int cls, KsRange q) {
  for (int g = 0; g < NGD; ++g)
    for (int r = 0; r < 16; ++r)
      if (p7b_tap_live(cls, r, g / CG / KS, g / CG % KS) && (g / 4 < q.lo || g / 4 >= q.hi)) return false;
  return q.lo >= 0 && q.hi <= KSD;
}
__host__ __device__ constexpr bool p7b_ranges_ok() {
  int sum = 0;
  for (int c = 0; c < MTD; ++c) {
    if (!p7b_range_covers(c, p7b_ks_range(c))) return false;
    sum += p7b_ks_range(c).hi - p7b_ks_range(c).lo;
  }
  return sum == 126;
}
constexpr bool ks_is(KsRange q, int lo, int hi) { return q.lo == lo && q.hi == hi; }
static_assert(MTD == 9 && NC1 % 16 == 0 && p7b_ranges_ok(), "conv2 dgrad: every live tap inside its class's range");
static_assert(ks_is(p7b_ks_range(0), 0, 7) && ks_is(p7b_ks_range(1), 0, 12) && ks_is(p7b_ks_range(2), 0, 15) &&
                  ks_is(p7b_ks_range(3), 0, KSD) && ks_is(p7b_ks_range(4), 0, KSD) &&
                  ks_is(p7b_ks_range(5), 0, KSD) && ks_is(p7b_ks_range(6), 3, KSD) &&
                  ks_is(p7b_ks_range(7), 7, KSD) && ks_is(p7b_ks_range(8), 12, KSD),
              "conv2 dgrad k-step ranges (rows 0-1, 1-2, 2-3, 4..7, 8-9, 9-10, 10-11)");
// the ranges packed 5 bits per class: a wave picks its own with scalar shifts
__host__ __device__ constexpr uint64_t p7b_pack(bool hi) {
  uint64_t v = 0;
  for (int c = 0; c < MTD; ++c)
    v |= static_cast<uint64_t>(hi ? p7b_ks_range(c).hi : p7b_ks_range(c).lo) << (5 * c);
  return v;
}
constexpr uint64_t P7B_LO = p7b_pack(false), P7B_HI = p7b_pack(true);
static_assert(KSD < 32 && MTD * 5 <= 64, "5-bit fields");
// conv2 backward wave map (P7).  Wave w runs on SIMD w % 4; waves 0 .. P7_DW - 1 take the data gradient, the other
// P7_DW the weight gradient, so every SIMD carries two waves of each role and both roles run side by side from the
// barrier after P6 to the one before P9.
// dgrad: a wave runs ONE tile class for all NI images, so its four tiles share one B fragment, one tap table entry
// and one bound check per k-step.  Classes 0 and MTD - 1 (disjoint 7-step ranges) share a wave, which runs class 0
// and then class MTD - 1.  The two dgrad waves of a SIMD (w, w + 4) are paired long with short: every SIMD carries
// 31-33 of the 126 k-steps (4 tiles each).
// wgrad: a wave owns NT2 = 2 of the 16 N-tiles (kidx columns) for both M-tiles: it reads its two A fragments
// once per k-step for both N-tiles.
constexpr int P7_DW = 8;       // dgrad waves 0..7, wgrad waves 8..15
constexpr int P7B_WCLS[P7_DW] = {3, 4, 5, 6, 1, 7, 0, 2};
constexpr int NT2 = 16 / (NW - P7_DW);  // conv2-wgrad N-tiles (250 -> 16 x 16) per wgrad wave
__host__ __device__ constexpr int p7a_tile(int w, int u) { return (w - P7_DW) * NT2 + u; }  // N-tile u of wave w
__host__ __device__ constexpr int p7b_wave_steps(int w) {  // k-steps of dgrad wave w (NI tiles per k-step)
  const int c = P7B_WCLS[w];
  int n = p7b_ks_range(c).hi - p7b_ks_range(c).lo;
  if (c == 0) n += p7b_ks_range(MTD - 1).hi - p7b_ks_range(MTD - 1).lo;
  return n;
}
__host__ __device__ constexpr bool p7b_map_ok() {
  // every (class, image) on exactly one dgrad wave: a wave covers all NI images of its class, and class MTD - 1
  // rides with class 0
  for (int c = 0; c < MTD; ++c)
    for (int im = 0; im < NI; ++im) {
      int n = 0;
      for (int w = 0; w < P7_DW; ++w)
        if (P7B_WCLS[w] == (c == MTD - 1 ? 0 : c)) ++n;
      if (n != 1) return false;
    }
  int tot = 0;
  for (int s = 0; s < 4; ++s) {  // a SIMD's dgrad k-steps inside the band, two waves of each role on it
    int n = 0, nd = 0, nw = 0;
    for (int w = s; w < NW; w += 4) {
      if (w < P7_DW) {
        n += p7b_wave_steps(w);
        ++nd;
      } else {
        ++nw;
      }
    }
    if (n < 31 || n > 33 || nd != 2 || nw != 2) return false;
    tot += n;
  }
  return tot == 126;
}
__host__ __device__ constexpr bool p7a_map_ok() {  // every (N-tile, M-tile) on exactly one wgrad wave
  for (int nt = 0; nt < 16; ++nt)
    for (int mt = 0; mt < 2; ++mt) {  // a wave runs both M-tiles of its N-tiles
      int n = 0;
      for (int w = P7_DW; w < NW; ++w)
        for (int u = 0; u < NT2; ++u)
          if (p7a_tile(w, u) == nt) ++n;
      if (n != 1) return false;
    }
  return true;
}
static_assert(NW == 16 && NI == 4 && p7b_map_ok(), "conv2 dgrad wave map: complete, balanced over the SIMDs");
static_assert(NT2 == 2 && NT2 * (NW - P7_DW) == 16 && p7a_map_ok(), "conv2 wgrad wave map: complete");
__host__ __device__ constexpr uint64_t p7b_pack_map() {
  uint64_t v = 0;
  for (int w = 0; w < P7_DW; ++w) v |= static_cast<uint64_t>(P7B_WCLS[w]) << (4 * w);
  return v;
}
constexpr uint64_t P7B_MCLS = p7b_pack_map();
// parameter offsets in the flat gradient (torch parameter order of Net)
constexpr int O_W1 = 0, O_B1 = O_W1 + W1N, O_W2 = O_B1 + C1, O_B2 = O_W2 + W2N, O_FC1W = O_B2 + C2,
              O_FC1B = O_FC1W + FC1N, O_FC2W = O_FC1B + F1, O_FC2B = O_FC2W + FC2N, NPARAM = O_FC2B + F2;
// Per-workgroup fp32 slabs hold every gradient EXCEPT fc1's weight (16,000 of the 21,840 parameters):
// that one is a rank-B product dW = dH^T . R2 over the whole batch, so each workgroup writes its 4 images'
// fc1 output gradients dH and inputs R2 (370 floats per image, K-contiguous) and k_cnn_reduce computes
// it as one f32-MFMA GEMM -- 1.5 MB of activations instead of 16 MB of slabs written and read back.
constexpr int NSLAB = NPARAM - FC1N;                     // 5,840 slab floats per workgroup
// (the slab's conv2-weight block [O_W2, O_W2 + W2N) holds dW2 as [co group of 4][kidx][4]: P7a's 16-byte
// stores of 16 consecutive kidx are 256 contiguous bytes; SLAB_OFS puts that block on a 128-byte line boundary
// and NSLABP pads each workgroup's slab to whole lines, so those stores are full-line writes)
static_assert(O_W2 % 4 == 0 && C2 % 4 == 0 && W2N % 4 == 0, "W2T: float4 columns of 4 co");
constexpr int SLAB_OFS = (32 - O_W2 % 32) % 32;                       // floats
constexpr int NSLABP = (SLAB_OFS + NSLAB + 31) / 32 * 32;             // slab pitch per workgroup (floats)
constexpr int S_FC1B = O_FC1B - FC1N, S_FC2W = O_FC2W - FC1N, S_FC2B = O_FC2B - FC1N;
constexpr int NACT = F1 + NIN;                           // activation rows: dH^T (50) then R2^T (320)
// row pitch (bf16 elements) of the activation image: the batch columns rounded up to 8 (16-byte operand loads)
__host__ __device__ constexpr int act_pitch(int nwg) { return (nwg * NI + 7) & ~7; }
static_assert(O_FC1W % 4 == 0 && FC1N % 4 == 0 && NSLAB % 4 == 0, "float4 slab columns");

__device__ __forceinline__ float hash_u01(unsigned long long seed, unsigned long long id) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ULL * (id + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  z ^= z >> 31;
  return static_cast<float>(z >> 40) * (1.0f / 16777216.0f);
}

__device__ __forceinline__ f32x4 mfma(const u16x8& a, const u16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                 0, 0);
}

// Cross-lane helpers on DPP row operations and lane reads: no LDS round trip (a __shfl_xor butterfly is a chain
// of dependent ds_bpermutes, ~0.1 us each: P4's softmax ran 15 of them back to back).  Whole wave active.
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float lanef(float v, int l) {  // l wave-uniform
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;
// every lane: op over the wave (quads, 8-lane halves, 16-lane rows by DPP, then the 4 rows' values by lane reads)
template <class Op>
__device__ __forceinline__ float wave_all(float v, Op op) {
  v = op(v, dppf<DPP_XOR1>(v));
  v = op(v, dppf<DPP_XOR2>(v));
  v = op(v, dppf<DPP_HALF_MIRROR>(v));
  v = op(v, dppf<DPP_MIRROR>(v));
  return op(op(lanef(v, 0), lanef(v, 16)), op(lanef(v, 32), lanef(v, 48)));
}
__device__ __forceinline__ float wave_sum_dpp(float v) { return wave_all(v, [](float a, float b) { return a + b; }); }
__device__ __forceinline__ float wave_max_dpp(float v) { return wave_all(v, [](float a, float b) { return fmaxf(a, b); }); }

struct CnnSmem {
  // bf16 MFMA operands
  alignas(16) uint16_t r1n[NI][NC1][C1P];  // relu(maxpool(conv1)) channel-last, ci padded with zeros (P1; read by
                                           // P2 and by P4's transpose into r1); e1 (P7b-P9) later, spanning r1n
                                           // and the front of w2f (r1n dead after P4, w2f after P2)
  alignas(16) u16x8 w2f[KS2][2][64];   // conv2 fwd B fragments [kstep][ntile][lane]
  alignas(16) u16x8 w2d[KSD][64];      // conv2 dgrad B fragments [kstep][lane]: B[k=(tap,co)][n=ci]
  alignas(16) u16x8 w1f[64];           // conv1 B fragment
  // conv2-output gradient (non-zero only at the argmax taps), twice: channel-last for the dgrad A
  // fragments (co padded to 32 with zeros) and as 8x8 planes for the wgrad A fragments.  Both are zeroed whole
  // in P0 (adjacent: one run of 16-byte stores) and have no other tenant until P9's partials alias d2n; P6
  // stores the live argmax taps only
  alignas(16) uint16_t d2n[NI * D2N_IM];     // (d2n_ofs layout)
  alignas(16) uint16_t d2[NI][C2][D2R];    // rows padded to 144 B: the 16 co rows of a wgrad A fragment hit
                                           // 16 distinct 16-B bank groups (128-B rows: 4-8-way conflicts)
  alignas(16) uint16_t zero16[8];      // 16 zero bytes: the target of every out-of-range operand read
  alignas(8) uint32_t p7tab[KSD * 4][2];  // P7b k-group g: {(ky << 16) | kx, d2n offset of the tap + co group}
  uint16_t x[NI][NXP];                 // images, rows of XP (columns 28.. zero)
  uint16_t xpad[18];                   // x1 starts 9 banks after x: P1 / P9 pixel-pair reads of x and x1 by
                                       // the same instruction no longer collide (8064-byte arrays)
  uint16_t x1[NI][NXP];                 // images shifted by one element (x1[i] = x[i + 1]): every pair of
                                       // consecutive pixels is ONE aligned 4-byte LDS read from x or x1
  uint16_t xonepad[48];                // xone starts 4 banks after x (36 words): P9's bias-column reads no longer
                                       // share a bank with the tap-(4,4) column (scripts/p9_lds_model.py)
  alignas(16) uint16_t xone[NI][NXP];  // bf16 1.0 everywhere: P9's B column 25 reads it (conv1's bias gradient)
  alignas(16) uint16_t r1[NI][C1 * RP16];   // relu(maxpool(conv1)), [ci][cell] (pitch RP16): P7a's B operand,
                                            // transposed from r1n inside P4 (the cells past NC1 are never written:
                                            // P7a's reads that touch them shift them out)
  // fp32 head
  alignas(16) float b1[C1];
  alignas(16) float b2[C2];
  alignas(16) float fc1b[F1];
  alignas(16) float fc2w[FC2N];
  alignas(16) float fc2b[F2];
  alignas(16) float r2[NI][NIN];       // fc1 input (NCHW flatten order); read as float4 in P3
  alignas(16) float dp2[NI][NIN];      // grad at the pooled conv2 output (dropout2d applied)
  float h1[NI][F1], m1[NI][F1], h1d[NI][F1];
  alignas(16) float dh[NI][DHP];       // rows padded to 16-byte multiples: P6 reads them as float4
  float mc2[NI][C2];
  float logit[NI][F2], dlog[NI][F2];
  float lossim[NI];                    // per-image loss terms (P4), summed at the end
  float valid[NI];
  int label[NI];
  alignas(16) unsigned char a1[NI][C1 * RP8];
  unsigned char a2[NI][NIN];
};
static_assert(sizeof(CnnSmem) <= 160 * 1024, "LDS budget");
static_assert((offsetof(CnnSmem, xone) - offsetof(CnnSmem, x)) / 4 % 32 == 4,
              "xone bank offset from x (P9 B reads: scripts/p9_lds_model.py; x1's: cnn_p1)");
static_assert(offsetof(CnnSmem, w2f) == offsetof(CnnSmem, r1n) + sizeof(uint16_t) * NI * NC1 * C1P &&
                  sizeof(uint32_t) * NI * C1 * EP <= sizeof(uint16_t) * NI * NC1 * C1P + sizeof(u16x8) * KS2 * 2 * 64,
              "e1 aliases r1n + w2f");
static_assert(offsetof(CnnSmem, d2n) == offsetof(CnnSmem, w1f) + sizeof(u16x8) * 64 &&
                  NW * 2 * 64 * sizeof(f32x4) <= sizeof(u16x8) * (KSD * 64 + 64) + sizeof(uint16_t) * NI * D2N_IM,
              "P9 partials alias w2d + w1f + d2n (not e1)");
static_assert(offsetof(CnnSmem, w2d) == offsetof(CnnSmem, w2f) + sizeof(u16x8) * KS2 * 2 * 64, "w2f, w2d adjacent");
constexpr int NFRAG = KS2 * 2 * 64 + KSD * 64 + 64;  // bf16 MFMA weight fragments (w2f, w2d, w1f)
constexpr int NF2F = KS2 * 2 * 64, NF2D = KSD * 64;  // fragment image: [w2f | w2d | w1f]
static_assert(NF2F <= 2 * T && NF2D <= 2 * T && NF2F + NF2D + 64 == NFRAG, "fragment slots");
static_assert(offsetof(CnnSmem, w1f) == offsetof(CnnSmem, w2d) + sizeof(u16x8) * KSD * 64, "w2d, w1f adjacent");
// fc1 forward: thread = (output j, 32-wide input chunk) over all images; fc1 backward dp2: thread = (input i,
// chunk of fc1 outputs).  Their partial sums live in the w2f region (dead after P2), combined in a fixed
// order (deterministic).
constexpr int FC1_KC = NIN / 32;        // 10 input chunks
constexpr int DP2_JC = 3;               // fc1-output chunks for dp2 (16, 16, 18 rows: float4-aligned starts)
constexpr int DP2_J = 16;               // rows per chunk (the last one takes the rest)
static_assert(F1 - DP2_J * (DP2_JC - 1) <= 20 && DP2_J % 4 == 0 && DHP >= DP2_J * (DP2_JC - 1) + 20, "dp2 chunks");
static_assert(F1 * FC1_KC <= T && NIN * DP2_JC <= T, "fc1 work split");
static_assert(sizeof(float) * NI * NIN * DP2_JC <= sizeof(u16x8) * KS2 * 2 * 64, "dp2 partials alias w2f");

// Workgroup barrier for LDS hand-offs only: every wave's LDS accesses complete (lgkmcnt), then s_barrier --
// outstanding GLOBAL loads and stores stay in flight (an LDS-scoped fence; __syncthreads would also wait
// vmcnt(0)).  Waves of k_cnn_train only exchange data through LDS: the slab / activation stores drain under
// the following phases and prefetched weights (w3, w6) arrive across barriers.
__device__ __forceinline__ void lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// An LDS address as the 32-bit offset a ds_read takes, and a 16-byte read at one: P7b selects between two
// addresses per read, which has to stay a select of integers (k_cnn_train)
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)(const __attribute__((address_space(3))) unsigned char*)(p);
#else
  return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p));
#endif
}
__device__ __forceinline__ u16x8 lds_read16(uint32_t o) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const __attribute__((address_space(3))) u16x8*)(o);
#else
  return u16x8{static_cast<uint16_t>(o), 0, 0, 0, 0, 0, 0, 0};
#endif
}

// Stores of the per-workgroup outputs the reduction launch reads (slabs, activation columns, loss partials):
// write-through (sc1), so the bytes leave the XCD's L2 under the remaining phases instead of at the kernel
// boundary (plain and non-temporal stores measured slower: profiles/r4k_cnn_store_modes.txt).  Vector stores only.
__device__ __forceinline__ void out_st(float* p, float v) {
  asm volatile("global_store_dword %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void out_st_u16x4(uint16_t* p, u16x4 v) { st_vec(reinterpret_cast<u16x4*>(p), v, true); }
__device__ __forceinline__ void out_st4(float* p, f32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}

// ---- P0 of k_cnn_train (TRAIN) and k_cnn_eval: images -> bf16 (x, x1), conv1's fragment, the fp32 head
// weights, the labels; TRAIN also the backward's constant tables and the dropout masks.
// ONE round trip: every value the phase takes from memory is requested before the first wait and the first
// LDS store -- conv1's fragment, the image quad, one head parameter per thread over the flat range
// [b1 | b2 | fc1b fc2w fc2b], rng[0] (a vector load: a scalar one would be a second trip behind the kernel
// arguments' wait) and the labels -- all unconditional, from clamped addresses; only the LDS stores are
// predicated (a load under `if (t < N)` becomes an exec branch with its own vmcnt(0): one dependent trip
// each).  conv2's forward fragments (fr, stored after conv1) are requested last: vmcnt retires in issue
// order, so P0's own waits are counted ones that leave them in flight.  The LDS fills that need no load run
// while the requests are out.  Image addresses are clamped to the batch; an empty slot holds zeros.
template <bool TRAIN, class Smem>
__device__ __forceinline__ void cnn_p0(Smem& S, int t, int n0, int B, const float* __restrict__ images,
                                       const int64_t* __restrict__ tgt, const float* __restrict__ params,
                                       const u16x8* __restrict__ frag, const unsigned long long* __restrict__ rng,
                                       float p_drop2, float p_drop1, int training, u16x8 (&fr)[2]) {
  static_assert(NI * NX / 4 <= T, "one image quad per thread");
  constexpr int NH = C1 + C2 + F1 + FC2N + F2;  // 590 head parameters, one per thread
  static_assert(NH <= T && O_FC2W == O_FC1B + F1 && O_FC2B == O_FC2W + FC2N, "fc1b, fc2w, fc2b contiguous");
  static_assert(offsetof(Smem, fc2b) == offsetof(Smem, fc2w) + sizeof(float) * FC2N, "fc2w, fc2b adjacent");
  static_assert((NI & (NI - 1)) == 0 && 384 % NI == 0, "label threads 384..: slot t & (NI - 1)");
  const int qi = min(t, NI * NX / 4 - 1);
  const int qim = (qi * 4) / NX, qoff = qi * 4 - qim * NX;
  const int hi = min(t, NH - 1);
  const int hsrc = hi < C1 ? O_B1 + hi : hi < C1 + C2 ? O_B2 + hi - C1 : O_FC1B + hi - (C1 + C2);
  const int lslot = t & (NI - 1);
  // the label address is selected, never the loaded value (tgt may be null in k_cnn_eval: any valid address)
  const int64_t* lbase = tgt != nullptr ? tgt : reinterpret_cast<const int64_t*>(frag);
  const int lidx = tgt != nullptr ? min(n0 + lslot, B - 1) : 0;
  // rng[0] through a per-lane offset the compiler cannot prove uniform: a global (vector) load
  int rofs = 0;
  asm("" : "+v"(rofs));
  // requests
  const u16x8 fw1 = frag[NF2F + NF2D + (t & 63)];
  const f32x4 img = *reinterpret_cast<const f32x4*>(images + static_cast<long>(min(n0 + qim, B - 1)) * NX + qoff);
  const float hv = params[hsrc];
  unsigned long long r0 = 0;
  if constexpr (TRAIN) r0 = rng[rofs];
  // (the int64 label's low word: what static_cast<int> keeps -- no half-dead register pair for the allocator
  // to reuse while the load is in flight, which costs a wait right here)
  const int lab = reinterpret_cast<const int*>(lbase)[2 * lidx];
  fr[0] = frag[t];
  fr[1] = frag[min(t + T, NF2F - 1)];
  // fills that need no load
  static_assert(H0 % 4 == 0 && XP >= H0 + 6, "image quads within a row; kx = 5 reads stay in the row");
  for (int i = t; i < NI * H0 * (XP - H0 + 1); i += T) {  // zero columns: x 28.., x1 27..
    const int r = i / (XP - H0 + 1), c = i - r * (XP - H0 + 1);
    if (c > 0) (&S.x[0][0])[r * XP + H0 - 1 + c] = 0;
    (&S.x1[0][0])[r * XP + H0 - 1 + c] = 0;
  }
  if constexpr (TRAIN) {
    // the conv2-output gradient, both layouts, zeroed whole: P6 then stores only the argmax taps.  d2n's extent
    // [0, NI D2N_IM) holds every slot a P7b A read can touch (co 20..23 and the row / position padding included),
    // d2 every row a P7a A read does; neither has another tenant before P9's partials
    constexpr int NZ = (sizeof(Smem::d2n) + sizeof(Smem::d2)) / 16;
    static_assert(offsetof(Smem, d2) == offsetof(Smem, d2n) + sizeof(Smem::d2n) && sizeof(Smem::d2n) % 16 == 0 &&
                      sizeof(Smem::d2) % 16 == 0 && NZ > T && NZ <= 2 * T,
                  "d2n, d2 adjacent: two 16-byte stores per thread");
    static_assert(sizeof(Smem::d2n) == sizeof(uint16_t) * NI * D2N_IM &&
                      d2n_ofs(NI - 1, O2 - 1, O2 - 1, CG * 8 - 1) == NI * D2N_IM - 1 && d2n_ofs(0, 0, 0, 0) == 0,
                  "d2n: the zeroed extent is first to last slot of (image, y, x, co < 24)");
    {
      u16x8* z = reinterpret_cast<u16x8*>(&S.d2n[0]);
      z[t] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (t + T < NZ) z[t + T] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    if (t < 8) S.zero16[t] = 0;
    static_assert((NI * NXP) % 8 == 0 && NI * NXP / 8 <= T, "xone: one 16-byte store per thread");
    if (t < NI * NXP / 8)
      reinterpret_cast<u16x8*>(&S.xone[0][0])[t] =
          u16x8{0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
    if (t < KSD * 4) {  // P7b's per-k-group tap table (groups past NGD never match: ky = kx = 0x8000)
      const int g = t, tap = g / CG, cg = g - tap * CG, ky = tap / KS, kx = tap - ky * KS;
      S.p7tab[g][0] = g < NGD ? (static_cast<uint32_t>(ky) << 16) | static_cast<uint32_t>(kx) : 0x80008000u;
      S.p7tab[g][1] = static_cast<uint32_t>(g < NGD ? (-(ky * D2N_RP + kx * D2N_P) + cg * D2N_Q) * 2 : 0);  // bytes
    }
  }
  // consumers, in request order
  if (t < 64) S.w1f[t] = fw1;
  if (t < NI * NX / 4) {
    const int im = qim, off = qoff, n = n0 + im;
    const f32x4 v = n < B ? img : f32x4{0.f, 0.f, 0.f, 0.f};
    const int row = off / H0, col = off - row * H0;  // a quad never crosses a row (H0 % 4 == 0)
    uint16_t* dst = &S.x[im][row * XP + col];
    const uint16_t b0 = f2bf(v[0]), b1 = f2bf(v[1]), b2 = f2bf(v[2]), b3 = f2bf(v[3]);
    dst[0] = b0; dst[1] = b1; dst[2] = b2; dst[3] = b3;
    uint16_t* d1 = &S.x1[im][row * XP + col];
    if (col > 0) d1[-1] = b0;
    d1[0] = b1; d1[1] = b2; d1[2] = b3;
  }
  if (t < NH) {  // fc2w and fc2b are adjacent in LDS as in params
    // (a byte offset, not a pointer select: that one becomes a branch per destination array)
    const int hofs = hi < C1             ? static_cast<int>(offsetof(Smem, b1)) + 4 * hi
                     : hi < C1 + C2      ? static_cast<int>(offsetof(Smem, b2)) + 4 * (hi - C1)
                     : hi < C1 + C2 + F1 ? static_cast<int>(offsetof(Smem, fc1b)) + 4 * (hi - (C1 + C2))
                                         : static_cast<int>(offsetof(Smem, fc2w)) + 4 * (hi - (C1 + C2 + F1));
    *reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(&S) + hofs) = hv;
  }
  if constexpr (TRAIN) {
    const unsigned long long seed = r0 * 0xD1B54A32D192ED03ULL;
    const float keep2 = training ? 1.f / (1.f - p_drop2) : 1.f;
    const float keep1 = training ? 1.f / (1.f - p_drop1) : 1.f;
    if (t < NI * C2) {
      const int im = t / C2, c = t - im * C2;
      const unsigned long long id = static_cast<unsigned long long>(n0 + im) * C2 + c;
      S.mc2[im][c] = (!training || hash_u01(seed ^ 0x5bd1e995ULL, id) >= p_drop2) ? keep2 : 0.f;
    } else if (t >= 128 && t < 128 + NI * F1) {
      const int u = t - 128, im = u / F1, j = u - im * F1;
      const unsigned long long id = static_cast<unsigned long long>(n0 + im) * F1 + j;
      S.m1[im][j] = (!training || hash_u01(seed ^ 0x27d4eb2fULL, id) >= p_drop1) ? keep1 : 0.f;
    }
  }
  if (t >= 384 && t < 384 + NI) {
    const bool ok = tgt != nullptr && n0 + lslot < B;
    if constexpr (TRAIN) S.valid[lslot] = ok ? 1.f : 0.f;
    S.label[lslot] = ok ? static_cast<int>(lab) : 0;
  }
}

// ---- The forward P1-P4 of k_cnn_train (TRAIN) and k_cnn_eval: ONE set of functions, so the two kernels run
// the same device code on the same operands in the same order -- their results agree bit for bit by
// construction.  TRAIN adds what only the backward reads (a1, a2, h1d) and the dropout masks; the backward's
// [ci][cell] copy of r1n (r1) is made later, inside P4, by waves that have nothing else to do there.

// max over a pooling window's 4 taps and the tap that holds it (the first tap wins a tie)
__device__ __forceinline__ float pool4(const f32x4& v, int& am) {
  am = 0;
  float m = v[0];
  if (v[1] > m) { m = v[1]; am = 1; }
  if (v[2] > m) { m = v[2]; am = 2; }
  if (v[3] > m) { m = v[3]; am = 3; }
  return m;
}

// conv1 tile ownership.  A tile is 4 consecutive pooling cells of one cell row (P1 / 4 tiles per row, MT1 per
// image).  Wave w owns NT1 CONTIGUOUS tiles: image w / P1_WI, the P1_WR whole cell rows from (w % P1_WI) * P1_WR,
// its tile u being row u / P1_TR of those, cells 4 (u % P1_TR) .. +3.  Only the wave's first tile depends on the
// wave id; tile u lies a compile-time distance from it in x, r1n and a1 alike.  (With the tiles dealt round
// robin, wid + u NW, none of that folded: every tile carried its own scalar tile / 36, t4 / 3 and remainder
// chains and its own vector address adds, ~650 issued instructions per wave around 9 MFMAs.)
static_assert(P1 % 4 == 0 && MT1 * 4 == NC1, "conv1 tiles: 4 cells of one row");
static_assert((NI * MT1) % NW == 0, "every wave runs the same number of conv1 tiles");
constexpr int NT1 = NI * MT1 / NW;  // 9 tiles per wave
constexpr int P1_TR = P1 / 4;       // 3 tiles per cell row
static_assert(MT1 % NT1 == 0, "conv1: a wave's tiles lie in one image");
static_assert(NT1 % P1_TR == 0, "conv1: a wave's tiles are whole cell rows");
constexpr int P1_WI = MT1 / NT1;    // 4 waves per image
constexpr int P1_WR = NT1 / P1_TR;  // 3 cell rows per wave
struct P1Tile {
  int im, py, px0;  // image, cell row, first cell column
};
__host__ __device__ constexpr P1Tile p1_tile(int w, int u) {
  return {w / P1_WI, (w % P1_WI) * P1_WR + u / P1_TR, (u % P1_TR) * 4};
}
__host__ __device__ constexpr bool p1_map_ok() {  // every (image, tile) on exactly one (wave, u)
  for (int tile = 0; tile < NI * MT1; ++tile) {
    int n = 0;
    for (int w = 0; w < NW; ++w)
      for (int u = 0; u < NT1; ++u) {
        const P1Tile q = p1_tile(w, u);
        if (q.im < 0 || q.im >= NI || q.py < 0 || q.py >= P1 || q.px0 < 0 || q.px0 + 4 > P1) return false;
        if (q.im * MT1 + q.py * P1_TR + q.px0 / 4 == tile) ++n;
      }
    if (n != 1) return false;
  }
  return true;
}
static_assert(p1_map_ok(), "conv1 wave map: the 16 waves cover each of the NI * MT1 tiles exactly once");

// ---- P1: conv1 (MFMA, M = (cell, tap), K = (ky, kx6) 30 -> 32, N = co) + maxpool2 + relu ----------
// K runs over 6-wide kernel rows (kx = 5 has zero weight): every k pair (kx even) is two consecutive
// pixels, read as ONE aligned 4-byte LDS load -- from x when the window starts on an even column (dx = 0),
// from the shifted copy x1 otherwise: 4 gathers per fragment instead of 8.
// Addresses: each lane forms its 4 gather bases and its 2 store bases (r1n, a1) ONCE, at the wave's first
// tile (p1_tile above); tile u's distance from it is a constant that rides in the LDS instruction's offset
// field, and pairs of gathers merge into ds_read2_b32.  The lane -> (cell, tap) mapping inside a tile, and
// with it the bank pattern of one gather instruction (2.75 LDS cycles, XP above), is the same for every tile.
template <bool TRAIN, class Smem>
__device__ __forceinline__ void cnn_p1(Smem& S, int lane, int wid) {
  static_assert((offsetof(Smem, x1) - offsetof(Smem, x)) / 4 % 32 == 9, "x1 bank offset from x (P1 gathers)");
  const int lr = lane & 15, lg = lane >> 4;
  int koff[4];  // pair p: k = 8 lg + 2p = (ky, kx) offset into the image; pairs past k = 30 read offset 0
                // (finite pixels times w1f's zero rows: no mask)
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int k = lg * 8 + 2 * p;
    koff[p] = k < KS * 6 ? (k / 6) * XP + (k % 6) : 0;
  }
  const u16x8 bw = S.w1f[lane];
  const int tap = lr & 3, dy = tap >> 1, dx = tap & 1;
  const uint16_t* xsrc = dx ? &S.x1[0][0] - 1 : &S.x[0][0];  // x1[i - 1] = x[i]: odd starts become even
  // the wave's first tile: image and cell row are wave-uniform (scalar, px0 = 0); the lane adds its cell
  // (lr >> 2), its tap and its 4 k pairs -- no per-lane division, nothing per tile
  const P1Tile w0 = p1_tile(wid, 0);
  const uint16_t* xlane = xsrc + dy * XP + 2 * (lr >> 2) + dx + w0.im * NXP + 2 * w0.py * XP;
  const uint16_t* xb[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) xb[p] = xlane + koff[p];
  // all of the wave's gathers first, then its MFMAs, then the epilogues: no tile waits on another's LDS
  // round trip (a one-tile-ahead pipeline measured 3.0 us for this loop, r4p)
  u16x8 ag[NT1];
#pragma unroll
  for (int u = 0; u < NT1; ++u) {
    const P1Tile q = p1_tile(0, u);  // tile u relative to the wave's first: constants once unrolled
    const int xo = 2 * q.py * XP + 2 * q.px0;
    u32x4 v;
#pragma unroll
    for (int p = 0; p < 4; ++p) v[p] = *reinterpret_cast<const uint32_t*>(xb[p] + xo);
    ag[u] = __builtin_bit_cast(u16x8, v);
  }
  f32x4 accs[NT1];
#pragma unroll
  for (int u = 0; u < NT1; ++u) accs[u] = mfma(ag[u], bw, f32x4{0.f, 0.f, 0.f, 0.f});
  const int co = lr;  // rows (lg*4 + r) = taps r of cell c0 + lg
  // (a clamped index and a select: no exec region around one LDS read)
  const float b1v = S.b1[min(co, C1 - 1)];
  const float bias1 = co < C1 ? b1v : 0.f;
  const int cw = w0.py * P1 + lg;  // the lane's cell of the wave's first tile; tile u's is q.py * P1 + q.px0 further
  uint16_t* r1n = &S.r1n[w0.im][cw][co];
  uint16_t rr[NT1];
  int am[NT1];
#pragma unroll
  for (int u = 0; u < NT1; ++u) {
    const P1Tile q = p1_tile(0, u);
    const float m = pool4(accs[u], am[u]);
    // lanes co >= C1: w1f's columns and bias1 are zero there, so r == 0 -- r1n's ci padding gets its zeros
    rr[u] = f2bf(fmaxf(m + bias1, 0.f));
    r1n[(q.py * P1 + q.px0) * C1P] = rr[u];
    if constexpr (TRAIN) {
      if (rr[u] == 0) am[u] = AM_DEAD;  // relu-dead: P7b's epilogue and P9 read the mask from a1
      // the tap is a VGPR value HERE: left alone, the compiler sinks the selects into the store region below
      // and keeps the 9 tiles' 27 compare masks (54 SGPRs) live up to it, which spills the kernel's long-lived
      // scalars to VGPR lanes
      asm volatile("" : "+v"(am[u]));
    }
  }
  if constexpr (TRAIN) {
    // the backward's copies, all tiles under ONE exec region: lanes co >= C1 have none (exec, no per-lane
    // address selects)
    if (co < C1) {
      unsigned char* a1 = &S.a1[w0.im][co * RP8 + cw];
#pragma unroll
      for (int u = 0; u < NT1; ++u) {
        const P1Tile q = p1_tile(0, u);
        a1[q.py * P1 + q.px0] = static_cast<unsigned char>(am[u]);
      }
    }
  }
}

// conv2 forward fragments (loaded in P0): bf16 MFMA order, straight 16-byte stores
template <class Smem>
__device__ __forceinline__ void cnn_store_w2f(Smem& S, int t, const u16x8 (&fr)[2]) {
  u16x8* dst = &S.w2f[0][0][0];
  dst[t] = fr[0];
  if (t + T < NF2F) dst[t + T] = fr[1];
}

// fc1's weights for P3 (32 per thread, 8 x 16-B L2 loads) are requested before conv2: their latency hides under
// it (registers: 78 -> ~110 VGPRs, no spill at 4 waves per SIMD)
__device__ __forceinline__ void cnn_fc1_rows(int t, const float* __restrict__ gFC1W, f32x4 (&w3)[8]) {
  if (t < F1 * FC1_KC) {
    const int j = t / FC1_KC, kc = t - j * FC1_KC;
    const f32x4* w4 = reinterpret_cast<const f32x4*>(gFC1W + j * NIN + kc * 4);
#pragma unroll
    for (int q = 0; q < 8; ++q) w3[q] = w4[q * (FC1_KC)];
  }
}

// ---- P2: conv2 (MFMA, M = (cell, tap) 64/image = 4 M-tiles, K = (ci,ky,kx) 250 -> 256, N = co 20 -> 32)
//          + dropout2d + maxpool2 + relu.  One (image, M-tile) per wave iteration, both N-tiles.
template <bool TRAIN, class Smem>
__device__ __forceinline__ void cnn_p2(Smem& S, int lane, int wid) {
  const int lr = lane & 15, lg = lane >> 4;
  for (int mtile = wid; mtile < NI * 4; mtile += NW) {
    const int im = mtile >> 2, mt = mtile & 3;
    const int tap = lr & 3, dy = tap >> 1, dx = tap & 1;
    const int cell = mt * 4 + (lr >> 2), py = cell >> 2, px = cell & 3;
    const int rb = (2 * py + dy) * P1 + 2 * px + dx;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    const uint16_t* r1n = &S.r1n[im][0][(lg & 1) * 8];
#pragma unroll
    for (int ks = 0; ks < KS2; ++ks) {
      const int tp = 2 * ks + (lg >> 1), ky = tp / KS, kx = tp - ky * KS;
      const u16x8 a = tp < KS * KS ? *reinterpret_cast<const u16x8*>(r1n + (rb + ky * P1 + kx) * C1P)
                                   : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      acc0 = mfma(a, S.w2f[ks][0][lane], acc0);
      acc1 = mfma(a, S.w2f[ks][1][lane], acc1);
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int co = nt * 16 + lr;
      if (co < C2) {
        int am;
        const float m = pool4(nt == 0 ? acc0 : acc1, am);
        const int q = co * NC2 + mt * 4 + lg;
        if constexpr (TRAIN) {
          S.r2[im][q] = fmaxf((m + S.b2[co]) * S.mc2[im][co], 0.f);
          S.a2[im][q] = static_cast<unsigned char>(am);
        } else {
          S.r2[im][q] = fmaxf(m + S.b2[co], 0.f);
        }
      }
    }
  }
}

// ---- P3: fc1 + relu + dropout.  Thread (j, kc): 32 weights of row j (8 x 16-B L2 loads, all in flight
// together) against the 4 images' inputs; partials [kc][im][j] summed in kc order. -------------------
template <bool TRAIN, class Smem>
__device__ __forceinline__ void cnn_p3(Smem& S, int t, const f32x4 (&w3)[8]) {
  static_assert(sizeof(float) * NI * F1 * FC1_KC <= sizeof(Smem::w2f), "fc1 partials alias w2f");
  float* part = reinterpret_cast<float*>(&S.w2f[0][0][0]);
  if (t < F1 * FC1_KC) {
    const int j = t / FC1_KC, kc = t - j * FC1_KC;
    // chunk kc = inputs {40 q + 4 kc .. +3 : q = 0..7}: the 10 chunks of a wave read 10 consecutive
    // float4s of r2 (conflict-free), and adjacent lanes load adjacent 16 B of the weight row (w3, loaded
    // before P2)
    const f32x4* w = w3;
    float s4[NI] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int im = 0; im < NI; ++im) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(&S.r2[im][q * 4 * FC1_KC + kc * 4]);
        s4[im] += w[q][0] * x[0] + w[q][1] * x[1] + w[q][2] * x[2] + w[q][3] * x[3];
      }
#pragma unroll
    for (int im = 0; im < NI; ++im) part[(kc * NI + im) * F1 + j] = s4[im];
  }
  lds_sync();
  if (t < NI * F1) {
    const int im = t / F1, j = t - im * F1;
    float s1 = S.fc1b[j];
#pragma unroll
    for (int kc = 0; kc < FC1_KC; ++kc) s1 += part[(kc * NI + im) * F1 + j];
    const float h = fmaxf(s1, 0.f);
    S.h1[im][j] = h;
    if constexpr (TRAIN) S.h1d[im][j] = h * S.m1[im][j];
  }
}

// ---- P4's head: fc2 logits and log_softmax of ONE image by ONE wave, no block barrier in between.
// Lane l < 4 F2 computes a quarter of logit v = l / 4 (rows j = l % 4 + 4 k), the quad sums it; the softmax
// reductions run across the wave's lanes (one thread per image summing serially took ~1.5 us).
// `h`: the fc1 output row of image slot `im` (h1d in training, h1 in evaluation).
struct CnnHead {
  float logit;  // lanes of quad v: logit v
  float lse;    // log-sum-exp of the 10 logits
  float ly;     // the label's logit
  int y;        // the label
};
template <class Smem>
__device__ __forceinline__ CnnHead cnn_head(const Smem& S, const float* h, int im, int lane) {
  static_assert(4 * F2 <= 64, "P4: a lane quad per logit");
  const int v = lane >> 2, p = lane & 3;
  const bool lv = v < F2;
  const int vr = lv ? v : 0;
  float s = 0.f;
  // (fully unrolled, like every loop between the w6 prefetch and P6: a loop header makes the compiler wait
  // for ALL outstanding global loads, w6 included)
#pragma unroll
  for (int k = 0; k < (F1 + 3) / 4; ++k) {
    const int j = p + 4 * k;
    if (j < F1) s += S.fc2w[vr * F1 + j] * h[j];
  }
  s += dppf<DPP_XOR1>(s);
  s += dppf<DPP_XOR2>(s);
  const float logit = s + S.fc2b[vr];
  const float m = wave_max_dpp(lv ? logit : -INFINITY);
  const float ex = __expf(logit - m);
  const float se = wave_sum_dpp(lv && p == 0 ? ex : 0.f);
  const float lse = m + __logf(se);
  const int y = S.label[im];  // (loaded in P0: a global load here would wait behind the w6 prefetch)
  const float ly = lanef(logit, __builtin_amdgcn_readfirstlane(4 * y));  // y: the wave's image label
  return {logit, lse, ly, y};
}

__global__ __launch_bounds__(T) void k_cnn_train(const float* __restrict__ images, const int64_t* __restrict__ tgt,
                                                 int B, const float* __restrict__ params,
                                                 const u16x8* __restrict__ frag,
                                                 const unsigned long long* __restrict__ rng, float p_drop2,
                                                 float p_drop1, int training, float* __restrict__ slabs,
                                                 float* __restrict__ loss_part, uint16_t* __restrict__ acts,
                                                 unsigned long long* __restrict__ stamps, int stop_after,
                                                 int fullk) {
  // optional phase timestamps (diagnostic only: stamps == nullptr in production launches); stop_after = k
  // ends the kernel after phase stamp k (diagnostic: hardware counters of a kernel prefix)
#define PDE_STAMP(k)                                                                      \
  if (stamps != nullptr && threadIdx.x == 0) stamps[blockIdx.x * 16 + (k)] = wall_clock64(); \
  if (stop_after == (k)) return
  // every argument P0 and the stamps read is live here: the kernel-argument segment arrives behind ONE wait
  // (left to the compiler, stamps / stop_after / fullk / frag each cost P0 a scalar round trip of their own)
  asm volatile("" ::"s"(images), "s"(tgt), "s"(B), "s"(params), "s"(frag), "s"(rng), "s"(p_drop2), "s"(p_drop1),
               "s"(training), "s"(slabs), "s"(loss_part), "s"(acts), "s"(stamps), "s"(stop_after), "s"(fullk),
               "s"(gridDim.x));
  PDE_STAMP(0);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  CnnSmem& S = *reinterpret_cast<CnnSmem*>(smem_raw);
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6);  // wave-uniform: scalar loop control / branches
  const int lr = lane & 15, lg = lane >> 4;  // fragment row/col (lane & 15) and k-group (lane >> 4)
  const float* gW1 = params + O_W1;
  const float* gW2 = params + O_W2;
  const float* gFC1W = params + O_FC1W;
  const int n0 = blockIdx.x * NI;

  // ---- P0 (cnn_p0): images -> bf16, conv1's bf16 MFMA fragment, fp32 head weights, dropout masks, tables.
  // Only w1f is stored to LDS now; conv2's forward fragments (w2f, fr) are requested in P0 and stored at the
  // end of P1, its data-gradient fragments (w2d) are requested ahead of P4 and stored inside it by the waves
  // that have no image there -- their latency is on no phase's critical path, and the burst of fragment reads
  // every workgroup makes at the start is 28 KB instead of 47 KB.  The conv2-output gradient planes (d2, d2n)
  // are zeroed here, while the loads are out.
  u16x8 fr[2];  // conv2 forward fragments: stored to LDS at the end of P1
  cnn_p0<true>(S, t, n0, B, images, tgt, params, frag, rng, p_drop2, p_drop1, training, fr);
  float* slab = slabs + static_cast<long>(blockIdx.x) * NSLABP + SLAB_OFS;
  lds_sync();
  PDE_STAMP(1);

  // ---- P1 .. P4's head: the forward shared with k_cnn_eval (cnn_p1 .. cnn_head above); the barriers and the
  // stamps between the phases stay here.  P1: conv1 + maxpool2 + relu
  cnn_p1<true>(S, lane, wid);
  if (stamps != nullptr) {  // diagnostic: conv1 done (waves 0 / 7 / 15), before the fragment stores
    if (t == 0) stamps[blockIdx.x * 16 + 13] = wall_clock64();
    if (t == 15 * 64) stamps[blockIdx.x * 16 + 15] = wall_clock64();
  }
  cnn_store_w2f(S, t, fr);
  lds_sync();
  PDE_STAMP(2);

  f32x4 w3[8];  // fc1's rows for P3, requested ahead of P2: conv2 + dropout2d + maxpool2 + relu
  cnn_fc1_rows(t, gFC1W, w3);
  cnn_p2<true>(S, lane, wid);
  lds_sync();
  PDE_STAMP(3);

  cnn_p3<true>(S, t, w3);  // P3: fc1 + relu + dropout
  lds_sync();
  PDE_STAMP(4);

  // conv2 data-gradient fragments for P7b, by the waves that have no image in P4 (TW threads, slots iw and
  // iw + TW): requested ahead of w6, so the counted wait in front of their LDS stores leaves w6 in flight, and
  // stored inside P4 while the head waves work (the w2d region is idle until P7b).  Under a wave-uniform branch
  // that only those waves take: loads every wave issued would sink into P4's branch, behind w6
  constexpr int TW = T - NI * 64;
  static_assert(NF2D > TW && NF2D <= 2 * TW, "w2d: two fragment slots per thread of the waves past the heads");
  const int iw = t - NI * 64;
  u16x8 fd[2];
  if (wid >= NI) {
    fd[0] = frag[NF2F + iw];
    fd[1] = frag[NF2F + min(iw + TW, NF2D - 1)];
  }
  // fc1 weight columns for P6's dp2 (thread (i, jc): up to 17 rows of column i), requested now so their L2
  // latency hides under P4 / P5
  // (unconditional loads from clamped addresses -- no divergent branch around them, so the compiler tracks
  // them precisely; rows past the chunk / threads past NIN x DP2_JC load a valid element whose sum P6 drops)
  constexpr int JPER = F1 - DP2_J * (DP2_JC - 1);  // 18: the longest chunk
  float w6[JPER];
  {
    const int tc = min(t, NIN * DP2_JC - 1);
    const int jc = tc / NIN, i = tc - jc * NIN;
#pragma unroll
    for (int u = 0; u < JPER; ++u) w6[u] = gFC1W[min(jc * DP2_J + u, F1 - 1) * NIN + i];
  }

  // ---- P4: fc2 logits, then log_softmax (cnn_head) + NLL + dlogits: ONE WAVE PER IMAGE.
  static_assert(NI <= NW, "P4: a wave per image");
  if (wid < NI) {
    const int im = wid, v = lane >> 2, p = lane & 3;
    const bool lv = v < F2;
    const auto [logit, lse, ly, y] = cnn_head(S, S.h1d[im], im, lane);
    const float val = S.valid[im];
    // d logit v of the image's own loss (lanes of quad v), NOT yet divided by B: every gradient below is linear
    // in it and passes through cnn_reduce_role, which applies 1 / B in fp32.  Scaled here, the bf16 operands
    // (dH, d2, e1) rounded v / B, so an image's contribution depended on the batch it came in unless B was a
    // power of two (for those, as the benchmark's, the scaling commutes with every rounding: same bits).
    const float dl = (__expf(logit - lse) - (v == y ? 1.f : 0.f)) * val;
    if (lv && p == 0) S.dlog[im][v] = dl;
    if (lane == 0) S.lossim[im] = val * (lse - ly);
    // P5's dh = relu'(h1) * mask * (W2^T dlog) of THIS image, in the same wave: lane j < F1 gathers the 10
    // d logits from the quads by shuffles (the fc2 weight / bias gradients, which sum over the images, are
    // taken in P6 after the barrier)
    static_assert(F1 <= 64, "P4: a lane per fc1 output");
    const int j = lane < F1 ? lane : 0;
    float sh = 0.f;
#pragma unroll
    for (int vv = 0; vv < F2; ++vv) sh += S.fc2w[vv * F1 + j] * lanef(dl, 4 * vv);
    if (lane < F1) S.dh[im][lane] = (S.h1[im][lane] > 0.f) ? sh * S.m1[im][lane] : 0.f;
  } else {
    // The waves without an image fill LDS regions that have no reader before P7a / P7b, while the LDS pipe is
    // nearly idle (straight-line code: a loop header would make the compiler drain w6).
    // r1, the [ci][cell] planes of P7a's B operand, transposed from the channel-last r1n (the same bf16 bits; r1n
    // is intact until P7b's epilogue).  Thread = (image, cell pair, channel half h): lane pairs read 32 contiguous
    // bytes, the two 16-byte reads (even cell, odd cell) are 2-way on the b128 lane groups; a store is the aligned
    // word {even cell, odd cell} of one channel, consecutive words over consecutive cell pairs.  Half 1 holds
    // channels 8, 9 and r1n's zero padding.
    static_assert(NC1 % 2 == 0 && RP16 % 2 == 0 && C1 > 8 && C1 <= 10 && C1P == 16 && NI * NC1 <= TW,
                  "r1 from r1n: cell pairs as aligned words, channels 0..7 | 8, 9");
    if (iw < NI * NC1) {
      const uint32_t uw = static_cast<uint32_t>(iw);  // (unsigned: the divisions are a multiply and shifts)
      const uint32_t im = uw / NC1, cp = (uw - im * NC1) >> 1, h = uw & 1;
      const uint32_t* src = reinterpret_cast<const uint32_t*>(&S.r1n[0][0][0]) + (uw >> 1) * C1P + h * 4;
      const u32x4 ev = *reinterpret_cast<const u32x4*>(src), od = *reinterpret_cast<const u32x4*>(src + C1P / 2);
      uint32_t* dst = reinterpret_cast<uint32_t*>(&S.r1[im][0]) + h * 8 * (RP16 / 2) + cp;
#pragma unroll
      for (int d = 0; d < 4; ++d)
        if (d == 0 || h == 0) {
          dst[(2 * d) * (RP16 / 2)] = (ev[d] & 0xFFFFu) | (od[d] << 16);
          dst[(2 * d + 1) * (RP16 / 2)] = (ev[d] >> 16) | (od[d] & 0xFFFF0000u);
        }
    }
    u16x8* dst = &S.w2d[0][0];
    dst[iw] = fd[0];
    if (iw + TW < NF2D) dst[iw + TW] = fd[1];
  }
  lds_sync();
  PDE_STAMP(5);
  PDE_STAMP(6);
  PDE_STAMP(7);

  // ---- P5 (fc2 backward) now lives in P4 (dh, per image) and P6 (the fc2 weight / bias gradients) -------

  // ---- P6: fc1 backward: dH / R2 columns for the batch-wide dW GEMM (k_cnn_reduce), db to the slab, and
  // dp2 = grad at the pooled conv2 output.  Columns n0..n0+3 of the K-contiguous bf16 [row][Bkp] image (the
  // reduction's bf16 MFMA operands): one 8-byte store per row (rows 0..49 dH^T, 50..369 R2^T); the workgroup
  // owning the last columns also zeroes the row padding up to Bkp (a multiple of 8).
  float* dpart = reinterpret_cast<float*>(&S.w2f[0][0][0]);  // [jc][im][i]
  // dp2's partial sums first: they are the phase's critical path, and w6's waits are counted ones that must not
  // see the write-through stores below (inline asm the compiler does not count: behind them the last w6 wait,
  // vmcnt(0), would wait for every store's acknowledgement).  Every thread consumes its w6 (clamped like the
  // loads; only the LDS stores are predicated), so no path reaches the rest of the kernel with loads pending
  {  // thread (i, jc): sum over fc1 outputs j in chunk jc (column loads coalesced)
    const int tc = min(t, NIN * DP2_JC - 1);
    const int jc = tc / NIN, i = tc - jc * NIN;
    const int j0 = jc * DP2_J, nj = jc == DP2_JC - 1 ? F1 - j0 : DP2_J;
    const float* w = w6;  // loaded before P4
    float s4[NI] = {0.f, 0.f, 0.f, 0.f};
    // dh read as float4 (5 per image instead of 18 scalars); products past the chunk are selected away
    // (the padding columns are never written: select, not multiply by zero)
#pragma unroll
    for (int im = 0; im < NI; ++im)
#pragma unroll
      for (int q = 0; q < (JPER + 3) / 4; ++q) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(&S.dh[im][j0 + 4 * q]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int u = 4 * q + e;
          if (u < JPER) s4[im] += u < nj ? w[u] * d[e] : 0.f;
        }
      }
    if (t < NIN * DP2_JC) {
#pragma unroll
      for (int im = 0; im < NI; ++im) dpart[(jc * NI + im) * NIN + i] = s4[im];
    }
  }
  static_assert(FC2N + F2 <= T, "fc2 weight / bias gradients: one element per thread");
  if (t < FC2N) {  // fc2 weight gradient (all images' dlog / h1d, complete since P4's barrier)
    const int v = t / F1, j = t - v * F1;
    float s = 0.f;
#pragma unroll
    for (int im = 0; im < NI; ++im) s += S.dlog[im][v] * S.h1d[im][j];
    out_st(&slab[S_FC2W + t], s);
  } else if (t < FC2N + F2) {
    const int v = t - FC2N;
    float s = 0.f;
#pragma unroll
    for (int im = 0; im < NI; ++im) s += S.dlog[im][v];
    out_st(&slab[S_FC2B + v], s);
  }
  {
    const int Bk = gridDim.x * NI, Bkp = act_pitch(gridDim.x);
    const bool pad = Bkp != Bk && n0 + NI == Bk;
    for (int row = t; row < NACT; row += T) {
      u16x4 v;
#pragma unroll
      for (int im = 0; im < NI; ++im) v[im] = f2bf(row < F1 ? S.dh[im][row] : S.r2[im][row - F1]);
      out_st_u16x4(acts + static_cast<long>(row) * Bkp + n0, v);
      if (pad) out_st_u16x4(acts + static_cast<long>(row) * Bkp + n0 + NI, u16x4{0, 0, 0, 0});
    }
  }
  if (t < F1) {
    float s = 0.f;
#pragma unroll
    for (int im = 0; im < NI; ++im) s += S.dh[im][t];
    out_st(&slab[S_FC1B + t], s);
  }
  lds_sync();
  // dp2 = grad at the pooled conv2 output, scattered to the argmax taps by the thread that combines it (both
  // layouts) -- no barrier between the two; the conv2 bias gradient, which needs every dp2 of a channel, runs
  // after the phase's closing barrier.  d2 and d2n were zeroed in P0: only the argmax tap of a live cell is
  // stored, 2 bytes in each layout (a dead cell's gradient is the zero already there).  ONE trip: thread (image
  // pair slot, q) takes the element q of images im0 and im0 + NI / 2, every LDS read of both items issued before
  // the first use
  constexpr int IH = NI / 2;
  static_assert(NI % 2 == 0 && IH * NIN <= T, "dp2 scatter: two images per thread, one trip");
  if (t < IH * NIN) {
    const int im0 = t / NIN, q = t - im0 * NIN, co = q / NC2, cell = q - co * NC2;
    const int py = cell >> 2, px = cell & 3;
    float pj[2][DP2_JC], rv[2], mk[2];
    int am[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int im = im0 + u * IH;
#pragma unroll
      for (int jc = 0; jc < DP2_JC; ++jc) pj[u][jc] = dpart[(jc * NI + im) * NIN + q];
      rv[u] = S.r2[im][q];
      mk[u] = S.mc2[im][co];
      am[u] = S.a2[im][q];
    }
    // (the values are VGPRs HERE: left alone, the compiler sinks an item's reads into its live-cell region below,
    // one dependent LDS round trip per item inside divergent code)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int jc = 0; jc < DP2_JC; ++jc) asm volatile("" : "+v"(pj[u][jc]));
      asm volatile("" : "+v"(rv[u]), "+v"(mk[u]), "+v"(am[u]));
    }
    float v[2];
    uint32_t o2[2], on[2];  // u16 index of the argmax tap in d2 / d2n
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int im = im0 + u * IH;
      float s1 = 0.f;
#pragma unroll
      for (int jc = 0; jc < DP2_JC; ++jc) s1 += pj[u][jc];
      v[u] = rv[u] > 0.f ? s1 * mk[u] : 0.f;
      S.dp2[im][q] = v[u];
      const int y = 2 * py + (am[u] >> 1), x = 2 * px + (am[u] & 1);
      o2[u] = static_cast<uint32_t>((im * C2 + co) * D2R + y * O2 + x);
      on[u] = static_cast<uint32_t>(d2n_ofs(im, y, x, co));
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (rv[u] > 0.f) {
        const uint16_t g = f2bf(v[u]);
        (&S.d2[0][0][0])[o2[u]] = g;
        S.d2n[on[u]] = g;
      }
  }
  lds_sync();
  PDE_STAMP(8);
  // ---- P7: conv2's backward, both gradients side by side from this barrier to the one before P9: waves P7_DW..
  // run the weight gradient (P7a), waves 0 .. P7_DW - 1 the data gradient (P7b) -- wave-uniform scalar branches
  // on wid, two waves of each role on every SIMD (the wave map above).
  // ---- P7a: conv2 wgrad (MFMA): dW2[co][(ci,ky,kx)] = sum_(im,y,x) d2[co][y][x] * r1[ci][y+ky][x+kx].
  // M = co (2 tiles), N = 250 -> 16 tiles (NT2 per wave), K = (im, y, x) 256 = 8 k-steps.  An A fragment
  // is one 16-byte row of the d2 plane, read once per k-step for the wave's NT2 N-tiles.
  if (wid >= P7_DW) {
    // Raised issue priority until the slab stores are out: the wgrad waves have the short job (8 k-steps), and
    // their write-through stores should leave early, to drain under the dgrad.  At equal priority they finish
    // late: the 8 -> 10 span is the same, but P9 runs 0.2-0.3 us longer and the kernel's end waits 0.6 us more
    // for the stores (profiles/cnn_p7_wave_roles.md)
    __builtin_amdgcn_s_setprio(3);
    constexpr int TB2 = (NW - 1) * 64;  // conv2 bias gradient: the first C2 lanes of the last wgrad wave
    static_assert(C2 <= 64 && NW - 1 >= P7_DW, "conv2 bias gradient on a wgrad wave");
    if (t >= TB2 && t < TB2 + C2) {  // (dp2 is not overwritten before P9)
      const int co = t - TB2;
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int im = 0; im < NI; ++im)
#pragma unroll
        for (int c = 0; c < NC2; c += 4) s4 += *reinterpret_cast<const f32x4*>(&S.dp2[im][co * NC2 + c]);
      out_st(&slab[O_B2 + co], (s4[0] + s4[1]) + (s4[2] + s4[3]));
    }
    // B gathers: the 8 consecutive u16 of a fragment start at a 2-byte-aligned address, so they are read as the
    // 5 aligned words covering them and funnel-shifted (v_alignbyte) when the start is odd -- one 16-byte read
    // there would be an unaligned LDS access (64 cycles), 8 masked u16 reads cost an exec round trip each
    // (columns kidx >= K2 and rows co >= C2 of the outputs are never stored: their lanes read real, finite
    // operands -- offset 0 / channel C2 - 1 -- instead of selecting zeros every k-step)
    int nb[NT2];
#pragma unroll
    for (int u = 0; u < NT2; ++u) {
      const int kidx = p7a_tile(wid, u) * 16 + lr, ci = kidx / 25, r = kidx - ci * 25, ky = r / 5, kx = r - ky * 5;
      nb[u] = kidx < K2 ? ci * RP16 + ky * P1 + kx : 0;
    }
    const uint16_t* arow[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) arow[mt] = &S.d2[0][min(mt * 16 + lr, C2 - 1)][0];
    f32x4 acc[2][NT2];
#pragma unroll
    for (int u = 0; u < NT2; ++u) acc[0][u] = acc[1][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < KSW2; ++ks) {
      const int im = ks >> 1, y = (ks & 1) * 4 + lg;  // this lane's 8 positions: row y, x = 0..7
      u16x8 a[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) a[mt] = *reinterpret_cast<const u16x8*>(arow[mt] + im * C2 * D2R + y * O2);
#pragma unroll
      for (int u = 0; u < NT2; ++u) {
        const int e0 = nb[u] + y * P1;  // first element
        // (index arithmetic, not pointer casts: the loads must stay LDS loads, not generic flat ones)
        const uint32_t* wp = reinterpret_cast<const uint32_t*>(&S.r1[im][0]) + (e0 >> 1);
        const uint32_t sh = static_cast<uint32_t>(e0 & 1) * 2;  // 0 or 2 bytes
        uint32_t w[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) w[q] = wp[q];
        u32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = __builtin_amdgcn_alignbyte(w[q + 1], w[q], sh);
        const u16x8 b = __builtin_bit_cast(u16x8, v);
        acc[0][u] = mfma(a[0], b, acc[0][u]);
        acc[1][u] = mfma(a[1], b, acc[1][u]);
      }
    }
    // the slab's conv2-weight block is kept as [co group][kidx][4] (see SLAB_OFS): a lane's 4 accumulator rows
    // are 4 consecutive co of one kidx, so they leave as one 16-byte store, and the 16 lanes of a co group write
    // 256 contiguous bytes (5000 dword stores per workgroup before; narrow write-through stores cost several
    // times the bytes' time, MI355X_MICROARCH.md store rows)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int u = 0; u < NT2; ++u) {
        const int kidx = p7a_tile(wid, u) * 16 + lr, cg = mt * 4 + lg;
        if (cg * 4 < C2 && kidx < K2) out_st4(&slab[O_W2 + (cg * K2 + kidx) * 4], acc[mt][u]);
      }
    __builtin_amdgcn_s_setprio(0);
  } else {
    // ---- P7b: conv2 dgrad (MFMA): dr1[ci][Y][X] = sum_(ky,kx) sum_co d2[Y-ky][X-kx][co] * w2[co][ci][ky][kx],
    // then relu'(r1).  M = r1 positions (9 tiles per image, 36 total), N = ci, K = (tap, co24) packed into 19
    // k-steps: a lane's A fragment is the 16-byte co-group of ITS tap's source position (Y-ky, X-kx), or the zero
    // block when that position lies outside the 8x8 conv2 output -- every read is unconditional, so the k-loop
    // pipelines its LDS reads ahead of the MFMAs.  A wave owns one tile class for all NI images (P7B_WCLS): its
    // four tiles cover the same positions, so they share the B fragment, the tap entry and the bound check of a
    // k-step, and the k-loop runs only the class's k-steps (p7b_ks_range: the others add exact zeros, so the sums
    // keep their bits).  Each tile has its own accumulator, summed over ascending k-steps.
    constexpr int MAXT = NI;
    const int cls0 = static_cast<int>(P7B_MCLS >> (4 * wid)) & 15;            // wave-uniform, scalar
    constexpr int im0 = 0;                                                    // images 0 .. NI - 1
    const int npass = cls0 == 0 ? 2 : 1;  // the class-0 wave goes on with class MTD - 1
    // LDS addresses as 32-bit offsets (the A reads select between two of them)
    const uint32_t sbase = lds_addr(smem_raw);
    const uint32_t zpo = sbase + static_cast<uint32_t>(offsetof(CnnSmem, zero16));  // the zero block
    constexpr uint32_t IMB = D2N_IM * 2;  // bytes between two images' slots
    // e1 aliases r1n / w2f, which no P7a / P7b wave reads (r1 itself is still P7a's B operand: no barrier here)
    uint32_t* e1 = reinterpret_cast<uint32_t*>(&S.r1n[0][0][0]);
    auto run_pass = [&](int pass) {
      const int cls = pass == 0 ? cls0 : MTD - 1;
      // (fullk: every class runs all KSD k-steps -- PDE_CNN_P7B_FULLK, diagnostic)
      const int lo = fullk ? 0 : static_cast<int>(P7B_LO >> (5 * cls)) & 31;
      const int hi = fullk ? KSD : static_cast<int>(P7B_HI >> (5 * cls)) & 31;
      // (4x4-block tiles model fewer bank conflicts, 6.8 -> 6.0 LDS cycles per A read, but measured slower:
      // P7b 5.76 -> 5.96 us, r4t)
      const int pos = cls * 16 + lr, ty = pos / P1, tx = pos - ty * P1;
      // (ty, tx) packed: one packed subtract checks both tap offsets
      const u16x2 tyx{static_cast<uint16_t>(tx), static_cast<uint16_t>(ty)};
      // LDS byte offset of tap (0,0), channel 0 of the first image: a k-step adds the tap offset and selects
      const uint32_t tpo = sbase + static_cast<uint32_t>(offsetof(CnnSmem, d2n)) + d2n_ofs(im0, ty, tx, 0) * 2;
      f32x4 acc[MAXT];
#pragma unroll
      for (int u = 0; u < MAXT; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      // the epilogue's argmax / dead marks of the lane's 4 cells, read ahead of the k-loop (rows ci >= C1 are
      // discarded: they read channel C1 - 1)
      const int ci = lr, cell = cls * 16 + lg * 4;
      uint32_t am4[MAXT];
#pragma unroll
      for (int u = 0; u < MAXT; ++u)
        am4[u] = *reinterpret_cast<const uint32_t*>(&S.a1[im0 + u][min(ci, C1 - 1) * RP8 + cell]);

      // k-step ks, lane group lg: tap / co group of k-group g = 4 ks + lg from the LDS table (one 8-byte read
      // instead of the divisions), validity of (Y - ky, X - kx) by one packed 16-bit subtract
      // (r4af: P7b was the phase with the most VALU instructions)
      // (table entries are read one k-step before the loads that use them: the read's latency hides under the
      // previous k-step's MFMAs)
      auto tab = [&](int ks) { return *reinterpret_cast<const u32x2*>(&S.p7tab[min(ks, KSD - 1) * 4 + lg][0]); };
      auto load = [&](const u32x2& e, u16x8 (&a)[MAXT]) {
        const u16x2 kyx = __builtin_bit_cast(u16x2, e[0]);
        const bool ok = (__builtin_bit_cast(uint32_t, static_cast<u16x2>(tyx - kyx)) & 0xFFF8FFF8u) == 0u;
        const uint32_t src = tpo + e[1];
#pragma unroll
        for (int u = 0; u < MAXT; ++u) {
          // the address is selected, never the loaded value (the empty asm keeps it a v_cndmask: with one
          // condition for both tiles the compiler otherwise branches around the reads and waits inside)
          uint32_t o = ok ? src + u * IMB : zpo;
          asm("" : "+v"(o));
          a[u] = lds_read16(o);
        }
      };
      // a scalar-counted loop over [lo, hi), two k-steps per trip on alternating operand registers (ae / be,
      // ao / bo): reads of k-step ks+1 are issued before the MFMAs of ks, one accumulator per tile in ascending
      // ks.  (The 19 steps unrolled, each under a wave-uniform lo <= ks < hi guard, index w2d / p7tab by
      // constants but measured no faster than without ranges: P7b 4.44 against 3.88 us, 34.5 against 28.1 KB
      // of code, profiles/r7_cnn_train_regs.md)
      u16x8 ae[MAXT], ao[MAXT], be, bo;
      load(tab(lo), ae);
      be = S.w2d[lo][lane];
      u32x2 en = tab(lo + 1);
      int ks = lo;
      for (; ks + 2 < hi; ks += 2) {  // straight-line trips: k-steps ks (ae, be), ks + 1 (ao, bo)
        u32x2 e = en;
        en = tab(ks + 2);
        load(e, ao);
        bo = S.w2d[ks + 1][lane];
#pragma unroll
        for (int u = 0; u < MAXT; ++u) acc[u] = mfma(ae[u], be, acc[u]);
        e = en;
        en = tab(ks + 3);
        load(e, ae);
        be = S.w2d[ks + 2][lane];
#pragma unroll
        for (int u = 0; u < MAXT; ++u) acc[u] = mfma(ao[u], bo, acc[u]);
      }
      if (ks + 1 < hi) {  // two k-steps left, or one
        load(en, ao);
        bo = S.w2d[ks + 1][lane];
#pragma unroll
        for (int u = 0; u < MAXT; ++u) acc[u] = mfma(ae[u], be, acc[u]);
#pragma unroll
        for (int u = 0; u < MAXT; ++u) acc[u] = mfma(ao[u], bo, acc[u]);
      } else {
#pragma unroll
        for (int u = 0; u < MAXT; ++u) acc[u] = mfma(ae[u], be, acc[u]);
      }
      // epilogue: the lane's 4 consecutive cells as e1 words (relu'(r1) from a1's dead mark), one 16-byte store
      if (ci < C1) {
#pragma unroll
        for (int u = 0; u < MAXT; ++u) {
          const int im = im0 + u;
          u32x4 e;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const uint32_t am = (am4[u] >> (8 * r)) & 0xFFu;
            e[r] = am == AM_DEAD ? 0u : static_cast<uint32_t>(f2bf(acc[u][r])) << (16 * (am & 1u));
          }
          *reinterpret_cast<u32x4*>(&e1[(im * C1 + ci) * EP + cell]) = e;
        }
      }
    };
    for (int pass = 0; pass < npass; ++pass) run_pass(pass);
  }
  PDE_STAMP(9);  // wave 0 (a dgrad wave) finished its P7 role
  lds_sync();
  PDE_STAMP(10);

  // ---- P9: conv1 wgrad (MFMA): dW1[co][(ky,kx)] = sum_(im,y,x) dconv1[co][y][x] * x[y+ky][x+kx], with
  // dconv1 = the pooled cell's gradient (e1) at its argmax tap.  M = co, N = 25 taps + the bias column (B = 1)
  // -> 2 tiles, K = (im, y, x) 2304 = 72 k-steps split over the waves; partials combined in LDS in a fixed order.
  // K order: a lane's 8 k-elements are 2 horizontally adjacent pooled cells x their 2x2 pooling windows, so its A
  // fragment is the 2 cells' e1 words placed by the argmax row (no per-position selects) and its B fragment 4
  // aligned pixel pairs (2 rows x 2 column pairs) of x or x1.
  {
    const uint16_t* xw[2];  // per N-tile column kidx: x (kx even) or x1 - 1 (kx odd) at the tap offset; the ones
                            // plane for the bias column 25; the discarded columns 26..31 read column 17's pixels
                            // (same addresses: a broadcast, no extra bank traffic)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k0 = u * 16 + lr, kidx = k0 > 25 ? 17 : k0;
      const int nb = (kidx / 5) * XP + kidx % 5;
      xw[u] = kidx == 25 ? &S.xone[0][0] : ((kidx % 5) & 1 ? &S.x1[0][0] - 1 : &S.x[0][0]) + nb;
    }
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const int co = lr;
    const int cr = co < C1 ? co : 0;  // rows co >= C1 are discarded: they read channel 0's (finite) data
    const uint32_t* e1 = reinterpret_cast<const uint32_t*>(&S.r1n[0][0][0]);
    // a fixed trip count (72 k-steps over 16 waves: 5 slots, the last one live on 8 waves -- a wave-uniform
    // skip): every slot's LDS reads are issued before the first select / MFMA
    constexpr int NK9 = (NI * KSW1 + NW - 1) / NW;
    static_assert(KSW1 * 4 * 2 == NC1 && P1 % 2 == 0, "P9: 4 lane groups x 2 cells per k-step");
    uint32_t m9[NK9];
    u32x2 e9[NK9];
    u16x8 b9[NK9][2];
#pragma unroll
    for (int u9 = 0; u9 < NK9; ++u9) {
      const int ks = wid + u9 * NW;
      if (ks >= NI * KSW1) break;  // wave-uniform
      const int im = ks / KSW1;
      const uint32_t gi = static_cast<uint32_t>((ks - im * KSW1) * 4 + lg);  // cell pair 0..71 of the image
      const uint32_t py = (gi * 43u) >> 8, pc = gi - py * 6u;               // gi / 6, gi % 6 (gi < 72)
      const int cell = static_cast<int>(py * P1 + pc * 2);
      m9[u9] = *reinterpret_cast<const uint16_t*>(&S.a1[im][cr * RP8 + cell]);
      e9[u9] = *reinterpret_cast<const u32x2*>(&e1[(im * C1 + cr) * EP + cell]);
      const int off = im * NXP + static_cast<int>(py * 2 * XP + pc * 4);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        // k order (dy, cell c, dx): pixel pairs (row 2py + dy, columns 4pc + 2c + {0, 1}), one ds_read2 per row
        // filling adjacent operand registers; never a 16-byte read at a 2-byte-aligned address, which the LDS
        // would replay as an unaligned access
        const uint16_t* src = xw[u] + off;
        u32x4 v;
        v[0] = *reinterpret_cast<const uint32_t*>(src);
        v[1] = *reinterpret_cast<const uint32_t*>(src + 2);
        v[2] = *reinterpret_cast<const uint32_t*>(src + XP);
        v[3] = *reinterpret_cast<const uint32_t*>(src + XP + 2);
        b9[u9][u] = __builtin_bit_cast(u16x8, v);
      }
    }
#pragma unroll
    for (int u9 = 0; u9 < NK9; ++u9) {
      if (wid + u9 * NW >= NI * KSW1) break;
      u32x4 a;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const bool lower = (m9[u9] >> (8 * c + 1)) & 1u;  // argmax in the window's second row (dead: e1 == 0)
        a[c] = lower ? 0u : e9[u9][c];
        a[2 + c] = lower ? e9[u9][c] : 0u;
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[u] = mfma(__builtin_bit_cast(u16x8, a), b9[u9][u], acc[u]);
    }
    // w2d / w1f / d2n are dead after P7b (its last reads precede the barrier before P9): the per-wave partials go
    // there without another barrier (e1, still read by slower waves, lies before them)
    f32x4* part = reinterpret_cast<f32x4*>(&S.w2d[0][0]);
    part[(wid * 2 + 0) * 64 + lane] = acc[0];
    part[(wid * 2 + 1) * 64 + lane] = acc[1];
    lds_sync();
    if (stamps != nullptr && t == 0) stamps[blockIdx.x * 16 + 14] = wall_clock64();  // diagnostic: partials in LDS
    // conv1's weight and bias gradients (slab [O_W1, O_B1 + C1), contiguous): thread t sums gradient t over the
    // waves in a fixed order (bias c = B column 25 of channel c), each quad gathers its 4 sums with DPP and its
    // first lane writes them as one 16-byte store (r4ac: dword stores cost the step ~0.8 us; a staging pass
    // through LDS cost a barrier, and separate bias waves summing dr1 another ~0.3 us)
    static_assert(O_W1 == 0 && O_B1 == W1N && (W1N + C1) % 4 == 0, "conv1 gradients: one float4 run");
    if (wid * 64 < W1N + C1) {  // wave-uniform: waves 0-4
      const bool live = t < W1N + C1;
      const int c = t < W1N ? t / 25 : (live ? t - W1N : 0);
      const int kidx = t < W1N ? t - c * 25 : 25;
      const int u = kidx >> 4;
      const int l = (c >> 2) * 16 + (kidx & 15), r = c & 3;
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) s += part[(w * 2 + u) * 64 + l][r];
      const int si = __builtin_bit_cast(int, s);
      const f32x4 q{s, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, si, 0x55, 0xF, 0xF, false)),
                    __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, si, 0xAA, 0xF, 0xF, false)),
                    __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, si, 0xFF, 0xF, 0xF, false))};
      if (live && (t & 3) == 0) out_st4(&slab[O_W1 + t], q);
    }
  }
  PDE_STAMP(11);

  // loss partial: the images' terms from P4
  if (wid == 0) {
    const float l = wave_sum_dpp(lane < NI ? S.lossim[lane] : 0.f);
    if (lane == 0) out_st(&loss_part[blockIdx.x], l);
  }
  if (stamps != nullptr) {  // diagnostic: every wave's stores drained, then the workgroup's last stamp
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    PDE_STAMP(12);
  }
}

// The conv weights in bf16 MFMA B-fragment order (conv2 fwd [ks][ntile][lane], conv2 dgrad [tap][lane],
// conv1 [lane]), written once per step so every training workgroup loads them with 16-byte copies.
__global__ __launch_bounds__(256) void k_cnn_prep(const float* __restrict__ params, u16x8* __restrict__ frag) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= NFRAG) return;
  const float* gW1 = params + O_W1;
  const float* gW2 = params + O_W2;
  u16x8 f;
  if (e < KS2 * 2 * 64) {  // conv2 fwd: B[k=(tap, ci16)][n=co] = w2[co][ci][tap]
    const int ks = e >> 7, nt = (e >> 6) & 1, l = e & 63;
    const int co = nt * 16 + (l & 15), g = l >> 4, tap = 2 * ks + (g >> 1), c8 = (g & 1) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      f[j] = (co < C2 && tap < KS * KS && c8 + j < C1) ? f2bf(gW2[co * K2 + (c8 + j) * KS * KS + tap]) : 0;
  } else if (e < KS2 * 2 * 64 + KSD * 64) {  // conv2 dgrad: B[k=(tap, co24)][n=ci] = w2[co][ci][tap]
    const int e2 = e - KS2 * 2 * 64, ks = e2 >> 6, l = e2 & 63;
    const int ci = l & 15, g = ks * 4 + (l >> 4), tap = g / CG, c0 = (g - tap * CG) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      f[j] = (g < NGD && ci < C1 && c0 + j < C2) ? f2bf(gW2[(c0 + j) * K2 + ci * 25 + tap]) : 0;
  } else {  // conv1: B[k = (ky, kx6)][n = co] = w1[co][ky][kx] (kx = 5 and k >= 30: zero)
    const int l = e - KS2 * 2 * 64 - KSD * 64;
    const int co = l & 15, k0 = (l >> 4) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + j, ky = k / 6, kx = k - ky * 6;
      f[j] = (co < C1 && k < KS * 6 && kx < KS) ? f2bf(gW1[co * 25 + ky * KS + kx]) : 0;
    }
  }
  frag[e] = f;
}

// Single-element inverse of k_cnn_prep: parameter p (flat index) with new value w -> its bf16 slot(s) in
// the fragment image (conv2 weights appear twice: forward and dgrad layouts; conv1 once; everything else
// is not staged).  Padding slots are never touched, so the image stays valid once k_cnn_prep wrote it.
__device__ __forceinline__ void write_frag(uint16_t* __restrict__ f, int p, float w) {
  const uint16_t b = f2bf(w);
  if (p >= O_W2 && p < O_W2 + W2N) {
    const int q = p - O_W2, co = q / K2, r = q - co * K2, ci = r / (KS * KS), tap = r - ci * (KS * KS);
    const int g = ((tap & 1) << 1) | (ci >> 3);
    const int e = ((tap >> 1) << 7) | ((co >> 4) << 6) | (g << 4) | (co & 15);  // conv2 fwd [ks][ntile][lane]
    f[e * 8 + (ci & 7)] = b;
    const int gd = tap * CG + (co >> 3);                                         // conv2 dgrad [kstep][lane]
    const int e2 = KS2 * 2 * 64 + (gd >> 2) * 64 + (((gd & 3) << 4) | ci);
    f[e2 * 8 + (co & 7)] = b;
  } else if (p >= O_W1 && p < O_W1 + W1N) {
    const int co = p / (KS * KS), k25 = p - co * (KS * KS);
    const int k = (k25 / KS) * 6 + k25 % KS;                                     // (ky, kx6) order
    const int e = KS2 * 2 * 64 + KSD * 64 + (((k >> 3) << 4) | co);             // conv1 [lane]
    f[e * 8 + (k & 7)] = b;
  }
}

// Plain SGD (torch.optim.SGD, momentum 0, no weight decay: mnist_horovod.py:50) on the flat parameters
// with the fragment image refreshed in the same pass, so the next step needs no k_cnn_prep.
// hp: the fused optimiser's device hyper-parameters (HP_LR, HP_GRAD_SCALE).
__global__ __launch_bounds__(256) void k_cnn_sgd(float* __restrict__ params, const float* __restrict__ grads,
                                                 const float* __restrict__ hp, uint16_t* __restrict__ frag,
                                                 int* __restrict__ step) {
  if (step != nullptr && blockIdx.x == 0 && threadIdx.x == 0) step[0] += 1;  // the optimiser's device step
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= NPARAM) return;
  const float w = params[p] - hp[HP_LR] * (grads[p] * hp[HP_GRAD_SCALE]);
  params[p] = w;
  write_frag(frag, p, w);
}

// grads (+)= 1 / B * (sum_wg slabs[wg] | dH^T . R2) in a fixed order (deterministic).
//  * slab blocks (blockIdx < RED_SLAB_BLOCKS): 8 waves over 16 float4 slab columns; lane = column + 16 x
//    slab-lane, so one load instruction of a wave reads 4 slabs x 256 B and each thread keeps nwg/32
//    independent float4 loads in flight;
//  * fc1 blocks: one 16 x 16 tile of dW_fc1[j][i] = sum_n dH[n][j] R2[n][i] on the bf16 matrix cores
//    (16x16x32, fp32 accumulation; the operands are the bf16 activation columns, like every other weight
//    gradient here -- fp32 columns with f32 MFMAs moved twice the bytes, r4u), the batch K split over the 8
//    waves, partials summed in wave order.  Lane (lr, lg) loads 16 B (8 columns) of row j (A) / row i (B) at
//    k = kb + 8 lg;
//  * block 0 also reduces the per-workgroup loss partials and advances the dropout RNG counter.
// With hp (single process, no all-reduce in between) every block also applies the SGD update to the
// parameters it reduced and refreshes their bf16 fragment slots.
constexpr int RED_COLS = 16;  // slab columns per reduce block (8: 183 blocks, measured slower, r4ag)
constexpr int RED_T = 512, RED_LANES = RED_T / RED_COLS;  // slab lanes per column
constexpr int NSLAB4 = NSLAB / 4;
constexpr int RED_SLAB_BLOCKS = (NSLAB4 + RED_COLS - 1) / RED_COLS;
constexpr int FC1_JT = (F1 + 15) / 16, FC1_IT = NIN / 16;   // 4 x 20 output tiles
constexpr int RED_BLOCKS = RED_SLAB_BLOCKS + FC1_JT * FC1_IT;
static_assert(NIN % 16 == 0, "fc1 input tiles");
static_assert(NI == 4, "activation columns are written as one 8-byte bf16 quad per row");

// w0 = params[p] and the hyper-parameters loaded at the start of the role (off the reduction's dependent chain)
__device__ __forceinline__ void sgd_update(float* params, float lr, float gsc, uint16_t* frag, int p, float w0,
                                           float g) {
  const float w = w0 - lr * (g * gsc);
  params[p] = w;
  write_frag(frag, p, w);
}

// One reduction role (rb = role block: slab columns for rb < RED_SLAB_BLOCKS, else an fc1 weight-gradient
// tile; role 0 also reduces the loss partials and advances the dropout RNG / SGD step counters), run by every
// thread of a RED_T block (block barriers inside): k_cnn_reduce, one role per block.
//
// OPT: the update the role applies when hp != nullptr.  0: plain SGD (sgd_update above; role 0 counts the step);
// 1: SGD with momentum and / or L2 weight decay; 2: Adam (L2); 3: AdamW -- optdev::update<OPT - 1> on the final
// gradient, the optimiser's state in the flat buffers om (momentum_buffer / exp_avg) and ov (exp_avg_sq, OPT >= 2),
// indexed like params and owned by the threads that own the weight.  These modes need the 1-based step: every
// block reads step[0] + 1 at role entry (one thread, a shared word, published by the role's own barrier) and
// arrives at the ticket in step[1] at its end; the last of gridDim.x arrivals stores the new count and clears the
// ticket (k_cnn_opt's protocol), so no block can read a count another block already advanced.
template <int OPT>
__device__ __forceinline__ void cnn_reduce_role(int rb, f32x4* part, uint32_t* s_epoch, int* s_fail,
                                                const float* __restrict__ slabs, int nwg,
                                                const uint16_t* __restrict__ acts, float* __restrict__ grads,
                                                int accumulate, const float* __restrict__ loss_part, int B,
                                                float* __restrict__ loss,
                                                unsigned long long* __restrict__ rng, float* __restrict__ params,
                                                const float* __restrict__ hp, uint16_t* __restrict__ frag,
                                                int* __restrict__ step, const XgmiView& xv, float xscale,
                                                float* __restrict__ om = nullptr, float* __restrict__ ov = nullptr) {
  const int tid = threadIdx.x;
  // always true in a RED_T block; the predicate stays because without it the compiler gives k_cnn_reduce<0> 84
  // VGPRs instead of 82 (profiles/r12_cnn_one_build.md)
  const bool act = tid < RED_T;
  int* s_stepw = nullptr;  // OPT != 0: the step being taken (1-based), one word per block
  int step0 = 0;
  if constexpr (OPT != 0) {
    __shared__ int s_step;
    s_stepw = &s_step;
  }
  // thread 0 requests the step count behind the first batch of operands (a vector load, like load_scalars') and
  // parks it in the shared word next to the partial sums: the role's barrier there publishes it to the updaters
  auto load_step = [&]() {
    if constexpr (OPT != 0) {
      int z = 0;
      asm("" : "+v"(z));
      if (tid == 0) step0 = step[z];
    }
  };
  auto park_step = [&]() {
    if constexpr (OPT != 0) {
      if (tid == 0) *s_stepw = step0 + 1;
    }
  };
  // the stateful update of parameter p (w0 / m0 / v0 loaded at the start of the role, g final) + fragment refresh
  auto opt_update = [&](const optdev::Hyper& h, int p, float w0, float m0, float v0, float g) {
    if constexpr (OPT != 0) {
      optdev::update<OPT - 1>(h, w0, g, m0, v0);
      params[p] = w0;
      om[p] = m0;
      if constexpr (OPT >= 2) ov[p] = v0;
      write_frag(frag, p, w0);
    }
  };
  // world > 1 with a peer view: this block's gradients go through the one-shot xGMI exchange (stage to my
  // slot, flags, read all ranks' values in rank order, x xscale) before the store + SGD update
  const bool xchg = xv.size > 1;
  // Each role requests its first batch of reduction operands (8 slab loads / 2 x CH activation loads) BEFORE
  // the small operands: the hyper-parameters and the owner's params / grads do not depend on the reduction and
  // are requested right behind that batch, as vector loads -- as scalar loads they were a wait for a memory
  // round trip in front of the first slab request.
  // k_cnn_train leaves its gradients unscaled (sums over the images, not means): 1 / B is applied here, in fp32
  const float inv_b = 1.f / static_cast<float>(B);
  float lrate = 0.f, gsc = 0.f;
  auto load_scalars = [&]() {
    int z = 0;  // a per-lane offset the compiler cannot prove uniform: global (vector) loads
    asm("" : "+v"(z));
    if (hp) {
      lrate = hp[HP_LR + z];
      gsc = hp[HP_GRAD_SCALE + z];
    }
  };
  const uint32_t epoch = xchg ? xgmi_epoch(xv, rb, s_epoch) : 0u;
  float* xmine = xchg ? xgmi_slot(xv, xv.rank, epoch) : nullptr;
  if (rb < RED_SLAB_BLOCKS) {
    const int col = tid % RED_COLS, sl = tid / RED_COLS;
    const int c4 = rb * RED_COLS + col;
    const f32x4* s4 = reinterpret_cast<const f32x4*>(slabs);
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
    const bool owner = act && sl == 0 && c4 < NSLAB4;
    // slab column -> parameter float4 (the xGMI staging index too); the conv2-weight block is [co group][kidx]
    // [4] in the slab (SLAB_OFS): its columns hold 4 co of one kidx, parameters K2 apart
    const int p4 = c4 < O_FC1W / 4 ? c4 : c4 + FC1N / 4;
    const bool w2t = c4 >= O_W2 / 4 && c4 < (O_W2 + W2N) / 4;
    int pj[4];
    {
      const int q = c4 - O_W2 / 4, cg = q / K2, kidx = q - cg * K2;
#pragma unroll
      for (int j = 0; j < 4; ++j) pj[j] = w2t ? O_W2 + (cg * 4 + j) * K2 + kidx : p4 * 4 + j;
    }
    // the first batch of 8 slab loads: unconditional, from clamped rows / columns (a thread without a full
    // batch adds zeros instead of the loaded values)
    const bool live = act && c4 < NSLAB4;
    const bool first = live && sl + 7 * RED_LANES < nwg;
    f32x4 v8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      v8[u] = s4[static_cast<long>(min(sl + u * RED_LANES, nwg - 1)) * (NSLABP / 4) + SLAB_OFS / 4 + min(c4, NSLAB4 - 1)];
    load_scalars();
    load_step();
    f32x4 w0 = a0, g0 = a0, m0 = a0, v0 = a0;
    // (one shape for both column kinds, four dword loads: with a float4 load on a second path the two paths'
    // results share registers, and the compiler drains the slab loads before it overwrites them)
    if (owner) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (hp) w0[j] = params[pj[j]];
        if (accumulate) g0[j] = grads[pj[j]];
        if constexpr (OPT != 0) {
          if (hp) m0[j] = om[pj[j]];
        }
        if constexpr (OPT >= 2) {
          if (hp) v0[j] = ov[pj[j]];
        }
      }
    }
    {
      const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
      a0 += first ? v8[0] + v8[4] : z4;
      a1 += first ? v8[1] + v8[5] : z4;
      a2 += first ? v8[2] + v8[6] : z4;
      a3 += first ? v8[3] + v8[7] : z4;
    }
    if (live) {
      int b = first ? sl + 8 * RED_LANES : sl;
      for (; b + 7 * RED_LANES < nwg; b += 8 * RED_LANES) {  // 8 independent loads in flight
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = s4[static_cast<long>(b + u * RED_LANES) * (NSLABP / 4) + SLAB_OFS / 4 + c4];
        a0 += v[0] + v[4];
        a1 += v[1] + v[5];
        a2 += v[2] + v[6];
        a3 += v[3] + v[7];
      }
      for (; b + 3 * RED_LANES < nwg; b += 4 * RED_LANES) {  // 4 in flight (nwg / RED_LANES < 8)
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = s4[static_cast<long>(b + u * RED_LANES) * (NSLABP / 4) + SLAB_OFS / 4 + c4];
        a0 += v[0];
        a1 += v[1];
        a2 += v[2];
        a3 += v[3];
      }
      for (; b < nwg; b += RED_LANES) a0 += s4[static_cast<long>(b) * (NSLABP / 4) + SLAB_OFS / 4 + c4];
    }
    if (act) part[sl * RED_COLS + col] = (a0 + a1) + (a2 + a3);
    park_step();
    __syncthreads();
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (owner) {
      v = part[col];
#pragma unroll 8
      for (int k = 1; k < RED_LANES; ++k) v += part[k * RED_COLS + col];
      v *= inv_b;
      if (xchg) reinterpret_cast<f32x4*>(xmine)[p4] = v;
    }
    bool ok = true;
    if (xchg) {
      ok = xgmi_publish_and_wait(xv, rb, epoch, s_fail);
      if (owner && ok) {
        f32x4 r4[kXgmiMaxRanks];
#pragma unroll
        for (int r = 0; r < kXgmiMaxRanks; ++r)
          if (r < xv.size) r4[r] = reinterpret_cast<const f32x4*>(xgmi_slot(xv, r, epoch))[p4];
        v = r4[0];
#pragma unroll
        for (int r = 1; r < kXgmiMaxRanks; ++r)
          if (r < xv.size) v += r4[r];
        v *= xscale;
      }
      xgmi_finish(xv, rb, epoch);
    }
    if (owner && ok) {
      if (accumulate) v += g0;
      if (w2t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) grads[pj[j]] = v[j];
      } else {
        reinterpret_cast<f32x4*>(grads)[p4] = v;
      }
      if constexpr (OPT == 0) {
        if (hp) {
#pragma unroll
          for (int j = 0; j < 4; ++j) sgd_update(params, lrate, gsc, frag, pj[j], w0[j], v[j]);
        }
      } else if (hp) {
        const optdev::Hyper h = optdev::load_hyper<OPT - 1>(hp, *s_stepw);
#pragma unroll
        for (int j = 0; j < 4; ++j) opt_update(h, pj[j], w0[j], m0[j], v0[j], v[j]);
      }
    }
  } else {
    const int fb = rb - RED_SLAB_BLOCKS;
    const int j0 = (fb / FC1_IT) * 16, i0 = (fb % FC1_IT) * 16;
    const int lane = tid & 63, wid = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const int Bkp = act_pitch(nwg);  // columns Bk.. are zero
    const int kper = ((Bkp + 8 * 32 - 1) / (8 * 32)) * 32;  // this wave's K slice, a multiple of 32
    const int k0 = wid * kper, k1 = act ? min(Bkp, k0 + kper) : k0;
    const bool jv = j0 + lr < F1;
    const uint16_t* arow = acts + static_cast<long>(jv ? j0 + lr : 0) * Bkp;
    const uint16_t* brow = acts + static_cast<long>(F1 + i0 + lr) * Bkp;
    constexpr int CH = 4;  // 32-deep chunks per pass: all 2 x CH loads in flight before the first MFMA
    const u16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
    // the first pass's 2 x CH operand loads: unconditional, from clamped columns (chunks past the wave's slice
    // and rows past F1 multiply as zeros, as in the loop below)
    u16x8 a1st[CH], b1st[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int k = k0 + 32 * c + 8 * lg;
      const int kc = k < k1 ? k : 0;
      a1st[c] = *reinterpret_cast<const u16x8*>(arow + kc);
      b1st[c] = *reinterpret_cast<const u16x8*>(brow + kc);
    }
    load_scalars();
    load_step();
    float w0[4] = {0.f, 0.f, 0.f, 0.f}, g0[4] = {0.f, 0.f, 0.f, 0.f};  // wave 0's outputs (j0 + 4 lg + r, i0 + lr)
    float m0[4] = {0.f, 0.f, 0.f, 0.f}, v0[4] = {0.f, 0.f, 0.f, 0.f};  // their optimiser state (OPT != 0)
    if (wid == 0 && act) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + lg * 4 + r;
        if (j < F1) {
          const int p = O_FC1W + j * NIN + i0 + lr;
          if (hp) w0[r] = params[p];
          if (accumulate) g0[r] = grads[p];
          if constexpr (OPT != 0) {
            if (hp) m0[r] = om[p];
          }
          if constexpr (OPT >= 2) {
            if (hp) v0[r] = ov[p];
          }
        }
      }
    }
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    // (an empty slice runs the first pass on zeros: the accumulators stay +0, as if skipped)
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const bool ok = k0 + 32 * c + 8 * lg < k1;
      a1st[c] = (ok && jv) ? a1st[c] : z8;
      b1st[c] = ok ? b1st[c] : z8;
    }
#pragma unroll
    for (int c = 0; c < CH; c += 2) {
      acc0 = mfma(a1st[c], b1st[c], acc0);
      acc1 = mfma(a1st[c + 1], b1st[c + 1], acc1);
    }
    for (int kb = k0 + 32 * CH; kb < k1; kb += 32 * CH) {
      u16x8 a[CH], b[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int k = kb + 32 * c + 8 * lg;  // 8 whole columns: k and Bkp are multiples of 8
        const bool ok = k < k1;
        a[c] = (ok && jv) ? *reinterpret_cast<const u16x8*>(arow + k) : z8;
        b[c] = ok ? *reinterpret_cast<const u16x8*>(brow + k) : z8;
      }
#pragma unroll
      for (int c = 0; c < CH; c += 2) {
        acc0 = mfma(a[c], b[c], acc0);
        acc1 = mfma(a[c + 1], b[c + 1], acc1);
      }
    }
    f32x4* wpart = part;
    if (act) wpart[wid * 64 + lane] = acc0 + acc1;
    park_step();
    __syncthreads();
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const int i = i0 + lr;
    if (wid == 0) {
      v = wpart[lane];
#pragma unroll
      for (int w = 1; w < RED_T / 64; ++w) v += wpart[w * 64 + lane];
      v *= inv_b;
      if (xchg) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = j0 + lg * 4 + r;
          if (j < F1) xmine[O_FC1W + j * NIN + i] = v[r];
        }
      }
    }
    bool ok = true;
    if (xchg) {
      ok = xgmi_publish_and_wait(xv, rb, epoch, s_fail);
      if (wid == 0 && ok) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = j0 + lg * 4 + r;
          const int p = O_FC1W + (j < F1 ? j : 0) * NIN + i;
          float a[kXgmiMaxRanks];
#pragma unroll
          for (int q = 0; q < kXgmiMaxRanks; ++q)
            if (q < xv.size) a[q] = xgmi_slot(xv, q, epoch)[p];
          float g = a[0];
#pragma unroll
          for (int q = 1; q < kXgmiMaxRanks; ++q)
            if (q < xv.size) g += a[q];
          v[r] = g * xscale;
        }
      }
      xgmi_finish(xv, rb, epoch);
    }
    if (wid == 0 && ok) {
      optdev::Hyper h{};
      if constexpr (OPT != 0) {
        if (hp) h = optdev::load_hyper<OPT - 1>(hp, *s_stepw);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + lg * 4 + r;
        if (j < F1) {
          const int p = O_FC1W + j * NIN + i;
          float g = v[r];
          if (accumulate) g += g0[r];
          grads[p] = g;
          if constexpr (OPT == 0) {
            if (hp) sgd_update(params, lrate, gsc, frag, p, w0[r], g);
          } else if (hp) {
            opt_update(h, p, w0[r], m0[r], v0[r], g);
          }
        }
      }
    }
  }
  if (rb == 0 && tid >= RED_T - 64 && tid < RED_T) {  // role 0's last wave: loss
    const int lane = tid - (RED_T - 64);
    float s = 0.f;
    for (int b = lane; b < nwg; b += 64) s += loss_part[b];
    s = wave_sum(s);
    if (lane == 0) {
      loss[0] = s / static_cast<float>(B);
      rng[0] += 1;  // advance the dropout stream for the next step
      if constexpr (OPT == 0) {
        if (hp != nullptr && step != nullptr) step[0] += 1;  // the fused SGD's device step counter
      }
    }
  }
  if constexpr (OPT != 0) {
    // every block read the old count before its arrival (a block whose exchange failed arrives too, or the
    // ticket would never clear); the last one publishes.  The next launch sees the stores across the kernel
    // boundary: a relaxed device-scope ticket is enough (optim_device.h run_chunks)
    __syncthreads();
    if (tid == 0) {
      const int prev = atomicAdd(step + 1, 1);
      if (prev == static_cast<int>(gridDim.x) - 1) {
        step[0] = step0 + 1;
        step[1] = 0;
      }
    }
  }
}

template <class A>
__device__ __forceinline__ void arg_live(A a) {
  asm volatile("" ::"s"(a));
}

// State: nothing for OPT 0 (plain SGD's kernel keeps exactly its arguments), else the two flat state pointers
// (float* om, float* ov) of cnn_reduce_role's stateful modes.
template <int OPT, class... State>
__global__ __launch_bounds__(RED_T) void k_cnn_reduce(const float* __restrict__ slabs, int nwg,
                                                      const uint16_t* __restrict__ acts, float* __restrict__ grads,
                                                      int accumulate, const float* __restrict__ loss_part, int B,
                                                      float* __restrict__ loss, unsigned long long* __restrict__ rng,
                                                      float* __restrict__ params, const float* __restrict__ hp,
                                                      uint16_t* __restrict__ frag, int* __restrict__ step,
                                                      XgmiView xv, float xscale, State... state) {
  static_assert(sizeof...(State) == (OPT != 0 ? 2 : 0), "the stateful modes take om and ov");
  __shared__ f32x4 part[RED_LANES * RED_COLS];  // slab: [lane][column]; fc1: [wave][lane] (same 8 KB)
  __shared__ uint32_t s_epoch;
  __shared__ int s_fail;
  // every argument live here: the kernel-argument segment arrives behind one wait, ahead of the first request
  asm volatile("" ::"s"(slabs), "s"(nwg), "s"(acts), "s"(grads), "s"(accumulate), "s"(loss_part), "s"(B), "s"(loss),
               "s"(rng), "s"(params), "s"(hp), "s"(frag), "s"(step), "s"(xv.size), "s"(xscale));
  (arg_live(state), ...);
  cnn_reduce_role<OPT>(blockIdx.x, part, &s_epoch, &s_fail, slabs, nwg, acts, grads, accumulate, loss_part, B, loss,
                       rng, params, hp, frag, step, xv, xscale, state...);
}

// ---------------------------------------------------------------------------------------------
// Forward-only evaluation: k_cnn_train's P0-P4 in eval mode (no dropout), nothing else.  The forward IS the
// training kernel's code, not a copy of it: cnn_p0 .. cnn_head instantiated without TRAIN, over the smaller LDS
// image below -- so a batch's summed NLL equals the training kernel's eval-mode loss x B; the outputs are the
// log-probabilities, their argmax and running totals.
//
// Geometry: NI = 4 images per 16-wave workgroup, as in training.  The forward is the same chain of short
// dependent phases, so it is latency-bound in the same way and 4 waves per image hide it; at the entry scripts'
// test batch of 1024 images that is 256 workgroups, one per CU -- 8 images per workgroup would leave half the
// chip idle for a pass that is one workgroup's latency long either way.  The LDS image is 69 KB (the training
// kernel's 122 KB less everything the backward keeps): two workgroups would fit a CU's LDS, but a second
// 16-wave workgroup needs 8 waves per SIMD, i.e. <= 64 VGPRs, and the kernel takes 72 (forcing 64 spills 8
// registers to scratch) -- so larger batches run one workgroup per CU, in rounds.
// ---------------------------------------------------------------------------------------------
struct CnnEvalSmem {
  alignas(16) uint16_t r1n[NI][NC1][C1P];  // relu(maxpool(conv1)) channel-last (CnnSmem::r1n)
  alignas(16) u16x8 w2f[KS2][2][64];       // conv2 B fragments; fc1's partials later (dead after conv2)
  alignas(16) u16x8 w1f[64];               // conv1 B fragment
  uint16_t x[NI][NXP];                     // images, rows of XP (CnnSmem::x / xpad / x1: same bank offsets)
  uint16_t xpad[18];
  uint16_t x1[NI][NXP];
  alignas(16) float b1[C1];
  alignas(16) float b2[C2];
  alignas(16) float fc1b[F1];
  alignas(16) float fc2w[FC2N];
  alignas(16) float fc2b[F2];
  alignas(16) float r2[NI][NIN];           // fc1 input; read as float4
  float h1[NI][F1];
  float lossim[NI];                        // -logp[y] per image (0 for an empty slot)
  int hit[NI];                             // pred == y per image (0 for an empty slot)
  int label[NI];
};
// (the layout conditions of the forward -- x1's bank offset, fc2w / fc2b adjacent, fc1's partials inside w2f --
// are asserted by cnn_p0 / cnn_p1 / cnn_p3 for every struct they are instantiated with)
static_assert(sizeof(CnnEvalSmem) <= 80 * 1024, "LDS budget");

// The running totals of CnnEvalStats (models/cnn_fused.py): four 8-byte words.
struct CnnEvalTotals {
  double loss_sum;              // sum of -logp[y]
  unsigned long long correct;   // predictions equal to the label
  unsigned long long count;     // images
  unsigned long long ticket;    // workgroups of the running launch that have arrived; 0 between launches
};
static_assert(sizeof(CnnEvalTotals) == 32, "CnnEvalStats holds int64[4]");

__global__ __launch_bounds__(T) void k_cnn_eval(const float* __restrict__ images, const int64_t* __restrict__ tgt,
                                                int B, const float* __restrict__ params,
                                                const u16x8* __restrict__ frag, float* __restrict__ logp,
                                                int64_t* __restrict__ pred, CnnEvalTotals* __restrict__ stats,
                                                float* __restrict__ loss_part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  CnnEvalSmem& S = *reinterpret_cast<CnnEvalSmem*>(smem_raw);
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
  const int n0 = blockIdx.x * NI;

  // ---- P0 (cnn_p0) without the backward's tables and the dropout masks; conv2's fragments (fr) are requested
  // there and stored after conv1
  asm volatile("" ::"s"(images), "s"(tgt), "s"(B), "s"(params), "s"(frag), "s"(logp), "s"(pred), "s"(stats),
               "s"(loss_part));  // the kernel arguments behind one wait
  u16x8 fr[2];
  cnn_p0<false>(S, t, n0, B, images, tgt, params, frag, nullptr, 0.f, 0.f, 0, fr);
  lds_sync();

  // ---- P1-P3: conv1 (only the channel-last r1n is kept), conv2, fc1, each + its pooling / relu, no dropout
  cnn_p1<false>(S, lane, wid);
  cnn_store_w2f(S, t, fr);
  lds_sync();
  f32x4 w3[8];
  cnn_fc1_rows(t, params + O_FC1W, w3);
  cnn_p2<false>(S, lane, wid);
  lds_sync();
  cnn_p3<false>(S, t, w3);
  lds_sync();

  // ---- P4: fc2 + log_softmax, one wave per image (cnn_head), then the outputs: the 10
  // log-probabilities, their argmax (lowest index on a tie) and the image's NLL / hit for the totals
  if (wid < NI) {
    const int im = wid, v = lane >> 2, p = lane & 3;
    const bool lv = v < F2;
    const auto [logit, lse, ly, y] = cnn_head(S, S.h1[im], im, lane);
    const float lp = logit - lse;
    const float best = wave_max_dpp(lv ? lp : -INFINITY);
    const float cand = (lv && lp == best) ? static_cast<float>(v) : static_cast<float>(F2);
    const int am = static_cast<int>(wave_all(cand, [](float a, float b) { return fminf(a, b); }));
    const int pr = am < F2 ? am : 0;  // (no lane equals the maximum only when the logits are NaN)
    const int n = n0 + im;            // wave-uniform
    const bool ok = n < B;
    if (ok && logp != nullptr && lv && p == 0) logp[static_cast<long>(n) * F2 + v] = lp;
    if (lane == 0) {
      if (ok && pred != nullptr) pred[n] = pr;
      S.lossim[im] = ok ? lse - ly : 0.f;  // == -logp[y]
      S.hit[im] = (ok && pr == y) ? 1 : 0;
    }
  }
  if (stats == nullptr) return;
  lds_sync();

  // ---- totals.  Every workgroup publishes its images' NLL sum and adds its hits (integer atomic); the
  // last one to draw a ticket sums the partials in workgroup order -- the same value whatever order the
  // workgroups finished in -- adds it to the running total and resets the ticket for the next launch or replay.
  if (wid == 0) {
    const float l = wave_sum_dpp(lane < NI ? S.lossim[lane] : 0.f);
    unsigned long long old = 0;
    if (lane == 0) {
      const int h = S.hit[0] + S.hit[1] + S.hit[2] + S.hit[3];
      __hip_atomic_store(&loss_part[blockIdx.x], l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (h != 0)
        __hip_atomic_fetch_add(&stats->correct, static_cast<unsigned long long>(h), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      old = __hip_atomic_fetch_add(&stats->ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned last = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(old));
    if (last == gridDim.x - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      float sum = 0.f;
      for (int b = lane; b < static_cast<int>(gridDim.x); b += 64)
        sum += __hip_atomic_load(&loss_part[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sum = wave_sum(sum);
      if (lane == 0) {
        stats->loss_sum += static_cast<double>(sum);
        stats->count += static_cast<unsigned long long>(B);
        __hip_atomic_store(&stats->ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

}  // namespace

int cnn_num_params() { return NPARAM; }
// PDE_CNN_P7B_FULLK=1 (diagnostic, read on every call): conv2's data gradient runs all KSD k-steps for every
// tile class instead of the class's own range (p7b_ks_range) -- the skipped steps add exact zeros, so the two
// must agree bit for bit.
static bool cnn_p7b_fullk_enabled() {
  const char* e = std::getenv("PDE_CNN_P7B_FULLK");
  return e != nullptr && e[0] == '1';
}

size_t cnn_frag_bytes() { return sizeof(u16x8) * NFRAG; }
size_t cnn_smem_bytes() { return sizeof(CnnSmem); }
int cnn_images_per_workgroup() { return NI; }

int cnn_slab_floats() { return NSLABP; }  // per workgroup, padded (SLAB_OFS)
int cnn_act_rows() { return NACT; }
int cnn_act_pitch(int nwg) { return act_pitch(nwg); }

bool cnn_update_valid(const CnnUpdate& u) {
  if (u.mode < CNN_SGD || u.mode > CNN_ADAMW) return false;
  if (u.mode == CNN_SGD) return true;
  return u.hp != nullptr && u.step != nullptr && u.m != nullptr && (u.mode < CNN_ADAM || u.v != nullptr);
}

hipError_t cnn_train_fused(const CnnTrainArgs& a, hipStream_t s) {
  const CnnUpdate& u = a.update;
  const int nwg = a.nwg;
  if (reinterpret_cast<uintptr_t>(a.grads) & 15) return hipErrorInvalidValue;  // float4 gradient stores
  if (!cnn_update_valid(u)) return hipErrorInvalidValue;
  XgmiView view{};
  view.size = 1;
  if (a.xv != nullptr && a.xv->size > 1) {
    // the exchange replaces the all-reduce of the gradients: no local accumulation in between, one flag
    // row and one staging float per parameter for each of this kernel's workgroups
    if (a.accumulate || a.xv->blocks < RED_BLOCKS || a.xv->slot_bytes < static_cast<int64_t>(NPARAM) * 4)
      return hipErrorInvalidValue;
    view = *a.xv;
  }
  const size_t sm = sizeof(CnnSmem);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cnn_train), hipFuncAttributeMaxDynamicSharedMemorySize,
                              static_cast<int>(sm));
    attr = true;
  }
  if (reinterpret_cast<uintptr_t>(a.frag) & 15) return hipErrorInvalidValue;
  if (a.prep)
    hipLaunchKernelGGL(k_cnn_prep, dim3(ceil_div(NFRAG, 256)), dim3(256), 0, s, a.params,
                       static_cast<u16x8*>(a.frag));
  if (reinterpret_cast<uintptr_t>(a.acts) & 15) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cnn_train, dim3(nwg), dim3(T), sm, s, a.images, a.tgt, a.B, a.params,
                     static_cast<const u16x8*>(a.frag), a.rng, a.p_drop2, a.p_drop1, a.training, a.slabs,
                     a.loss_part, a.acts, a.stamps, a.stop_after, cnn_p7b_fullk_enabled() ? 1 : 0);
  uint16_t* fr = static_cast<uint16_t*>(a.frag);
  if (u.mode == CNN_SGD) {  // (no state arguments: k_cnn_reduce<0>'s pack is empty)
    hipLaunchKernelGGL(k_cnn_reduce<0>, dim3(RED_BLOCKS), dim3(RED_T), 0, s, a.slabs, nwg, a.acts, a.grads,
                       a.accumulate, a.loss_part, a.B, a.loss, a.rng, a.params, u.hp, fr, u.step, view, a.xscale);
  } else {
    using ReduceFn = decltype(&k_cnn_reduce<1, float*, float*>);
    static const ReduceFn kReduce[3] = {&k_cnn_reduce<1, float*, float*>, &k_cnn_reduce<2, float*, float*>,
                                        &k_cnn_reduce<3, float*, float*>};
    hipLaunchKernelGGL(kReduce[u.mode - CNN_SGD_STATE], dim3(RED_BLOCKS), dim3(RED_T), 0, s, a.slabs, nwg, a.acts,
                       a.grads, a.accumulate, a.loss_part, a.B, a.loss, a.rng, a.params, u.hp, fr, u.step, view,
                       a.xscale, u.m, u.v);
  }
  return hipGetLastError();
}

int cnn_eval_images_per_workgroup() { return NI; }

hipError_t cnn_eval_fused(const float* images, const int64_t* tgt, int B, const float* params, void* frag,
                          float* logp, int64_t* pred, void* stats, float* loss_part, int prep, hipStream_t s) {
  if (B < 1 || (reinterpret_cast<uintptr_t>(frag) & 15) || (reinterpret_cast<uintptr_t>(stats) & 7))
    return hipErrorInvalidValue;
  if (stats != nullptr && (tgt == nullptr || loss_part == nullptr)) return hipErrorInvalidValue;
  const size_t sm = sizeof(CnnEvalSmem);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cnn_eval), hipFuncAttributeMaxDynamicSharedMemorySize,
                              static_cast<int>(sm));
    attr = true;
  }
  if (prep)
    hipLaunchKernelGGL(k_cnn_prep, dim3(ceil_div(NFRAG, 256)), dim3(256), 0, s, params, static_cast<u16x8*>(frag));
  hipLaunchKernelGGL(k_cnn_eval, dim3(ceil_div(B, NI)), dim3(T), sm, s, images, tgt, B, params,
                     static_cast<const u16x8*>(frag), logp, pred, static_cast<CnnEvalTotals*>(stats), loss_part);
  return hipGetLastError();
}

// The stateful updates (torch.optim's SGD with momentum / weight decay, Adam, AdamW -- the last is the Horovod-elastic
// script's optimiser, horovod_mnist_elastic.py:41) on the flat parameters, their state as flat buffers, with the
// fragment image refreshed in the same pass -- the multi-tensor update launch and the next step's fragment prep
// launch become ONE launch.  hp / step: the fused optimiser's device hyper-parameters and {steps taken, arrival
// counter}, read and advanced exactly as its own update kernel does (optim_device.h run_chunks), so its state_dict
// and later steps stay consistent.
//
// MODE: optdev's (0 SGD with momentum and / or L2 weight decay -- m: the momentum buffers, v unused; 1 Adam with
// L2; 2 AdamW), one less than the CnnUpdateMode.  The updates after an all-reduce that did not run inside the slab
// reduction (RCCL, the fusion engine, DDP); plain SGD keeps k_cnn_sgd.
template <int MODE>
__global__ __launch_bounds__(256) void k_cnn_opt(float* __restrict__ params, const float* __restrict__ grads,
                                                 float* __restrict__ m, float* __restrict__ v,
                                                 const float* __restrict__ hp, int* __restrict__ step,
                                                 uint16_t* __restrict__ frag) {
  __shared__ int s_step;
  if (threadIdx.x == 0) s_step = step[0] + 1;
  __syncthreads();
  const optdev::Hyper h = optdev::load_hyper<MODE>(hp, s_step);
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < NPARAM) {
    float w = params[p], mm = m[p], vv = 0.f;
    if constexpr (MODE != 0) vv = v[p];
    optdev::update<MODE>(h, w, grads[p], mm, vv);
    params[p] = w;
    m[p] = mm;
    if constexpr (MODE != 0) v[p] = vv;
    write_frag(frag, p, w);
  }
  __syncthreads();  // (every block read the old count before its arrival: the last one publishes)
  if (threadIdx.x == 0) {
    const int prev = atomicAdd(step + 1, 1);
    if (prev == static_cast<int>(gridDim.x) - 1) {
      step[0] = s_step;
      step[1] = 0;
    }
  }
}

hipError_t cnn_opt_fused(float* params, const float* grads, void* frag, const CnnUpdate& u, hipStream_t s) {
  if (!cnn_update_valid(u) || u.hp == nullptr || (reinterpret_cast<uintptr_t>(frag) & 15))
    return hipErrorInvalidValue;
  uint16_t* fr = static_cast<uint16_t*>(frag);
  if (u.mode == CNN_SGD) {
    hipLaunchKernelGGL(k_cnn_sgd, dim3(ceil_div(NPARAM, 256)), dim3(256), 0, s, params, grads, u.hp, fr, u.step);
  } else {
    using OptFn = decltype(&k_cnn_opt<2>);
    // the one place the CnnUpdateMode becomes optdev's MODE
    static const OptFn kOpt[3] = {&k_cnn_opt<0>, &k_cnn_opt<1>, &k_cnn_opt<2>};
    hipLaunchKernelGGL(kOpt[u.mode - CNN_SGD_STATE], dim3(ceil_div(NPARAM, 256)), dim3(256), 0, s, params, grads,
                       u.m, u.v, u.hp, u.step, fr);
  }
  return hipGetLastError();
}

// ---- hvd.Adasum of the weight DELTAS (hvd/optimizer.py _adasum_step), two launches behind forward_backward ----
// Per rank r: delta_r = local_update(start, g_r, state_r) - start, and w = start + adasum_r(delta_r) with one set of
// coefficients per parameter TENSOR (adasum_weights.h).  Both launches run k_cnn_opt's decomposition -- one parameter
// per thread, ceil(NPARAM / 256) workgroups of 256, the same on every rank -- so a workgroup's 256-element chunk is
// what it stages, what it reads from the peers and what it updates.  A PIECE is (tensor s) x (chunk b); its partial
// Gram goes to workspace row b + s (k_xgmi_adasum_gram's numbering, xgmi_allreduce.hip: unique, the rows of one tensor
// contiguous).  The Gram and combine arithmetic are that file's (fp64 sums of exact products in a fixed order, fp32
// weights, rank-order fmas), written out again here for the one-element-per-thread layout: the stand-alone kernels
// stay as they are.
constexpr int ADA_T = 256, ADA_WAVES = ADA_T / 64, ADA_NSEG = 8;
constexpr int ADA_BLOCKS = (NPARAM + ADA_T - 1) / ADA_T;
struct CnnSegEnds {
  int end[ADA_NSEG];  // cumulative element ends of Net's parameter tensors in the flat buffer
};
constexpr CnnSegEnds kCnnSegEnds = {{O_B1, O_W2, O_B2, O_FC1W, O_FC1B, O_FC2W, O_FC2B, NPARAM}};

// Launch A.  MODE: the CnnUpdateMode; NR: the world size.  The local update with the optimiser's own functions
// (sgd_update's expression / optdev::update), state stored, the weight NOT: params keeps `start` for launch B, so
// no copy of the starting weights exists.  The delta is staged in this rank's slot, exchanged (xgmi_device.h), and
// every piece's Gram over all ranks' slots is accumulated in fp64: per thread one element, wave shuffle, the
// workgroup's waves in order -- no floating-point atomics, the same bits on every rank.  Then k_cnn_opt's step ticket.
template <int MODE, int NR>
__global__ __launch_bounds__(ADA_T) void k_cnn_adasum_delta(const float* __restrict__ params,
                                                            const float* __restrict__ grads, float* __restrict__ m,
                                                            float* __restrict__ v, const float* __restrict__ hp,
                                                            int* __restrict__ step, XgmiView xv, CnnSegEnds segs,
                                                            double* __restrict__ gram) {
  constexpr int NG = NR * (NR + 1) / 2;
  __shared__ uint32_t s_epoch;
  __shared__ int s_fail;
  __shared__ int s_step;
  __shared__ double s_part[ADA_WAVES][NG];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid == 0) s_step = step[0] + 1;
  const uint32_t epoch = xgmi_epoch(xv, b, &s_epoch);  // (its barrier publishes s_step too)
  const int p = b * ADA_T + tid;
  const bool live = p < NPARAM;
  if constexpr (MODE == CNN_SGD) {
    if (live) {
      const float w0 = params[p];
      const float w1 = w0 - hp[HP_LR] * (grads[p] * hp[HP_GRAD_SCALE]);
      xgmi_slot(xv, xv.rank, epoch)[p] = w1 - w0;
    }
  } else {
    const optdev::Hyper h = optdev::load_hyper<MODE - 1>(hp, s_step);
    if (live) {
      const float w0 = params[p];
      float w1 = w0, mm = m[p], vv = 0.f;
      if constexpr (MODE >= CNN_ADAM) vv = v[p];
      optdev::update<MODE - 1>(h, w1, grads[p], mm, vv);
      m[p] = mm;
      if constexpr (MODE >= CNN_ADAM) v[p] = vv;
      xgmi_slot(xv, xv.rank, epoch)[p] = w1 - w0;
    }
  }
  if (xgmi_publish_and_wait(xv, b, epoch, &s_fail)) {
    xgmi_read_delay(xv);
    float x[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) x[r] = live ? xgmi_slot(xv, r, epoch)[p] : 0.f;
    const int lo = b * ADA_T;
    const int hi = lo + ADA_T < NPARAM ? lo + ADA_T : NPARAM;
    int s = 0;
    while (s < ADA_NSEG - 1 && segs.end[s] <= lo) ++s;  // the first tensor that reaches into this chunk
    for (int plo = lo; plo < hi && s < ADA_NSEG; ++s) {
      const int phi = segs.end[s] < hi ? segs.end[s] : hi;
      const bool in = p >= plo && p < phi;
      double g[NG];
      {
        int k = 0;
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
          for (int j = i; j < NR; ++j)
            g[k++] = in ? static_cast<double>(x[i]) * static_cast<double>(x[j]) : 0.0;
      }
#pragma unroll
      for (int k = 0; k < NG; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) g[k] += __shfl_down(g[k], off, 64);
      }
      if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NG; ++k) s_part[tid >> 6][k] = g[k];
      }
      __syncthreads();
      if (tid < NG) {
        double t = s_part[0][tid];
#pragma unroll
        for (int w = 1; w < ADA_WAVES; ++w) t += s_part[w][tid];
        gram[static_cast<int64_t>(b + s) * kXgmiGramRow + tid] = t;
      }
      __syncthreads();  // s_part is reused by the next piece
      plo = phi;
    }
  }
  xgmi_finish(xv, b, epoch);
  // (every block read the old count before its arrival: the last one publishes -- k_cnn_opt's protocol)
  if (tid == 0) {
    const int prev = atomicAdd(step + 1, 1);
    if (prev == static_cast<int>(gridDim.x) - 1) {
      step[0] = s_step;
      step[1] = 0;
    }
  }
}

// Launch B.  It re-reads the peers' slots of the call launch A exchanged: the two-slot lifetime argument above
// k_xgmi_adasum_combine (xgmi_allreduce.hip) covers this second launch unchanged.  The epoch is the one launch A's
// xgmi_finish stored; a set error word means some chunk's Gram or bytes are missing, and nothing is written.  Every
// workgroup sums the partial rows of the tensors it touches in row order and derives the weights with the same code
// from the same bits, on every rank; w = start + (w_0 x_0, then fmas in rank order), and the bf16 fragment slots of
// the new weight are refreshed, so the next step needs no prep launch.
template <int NR>
__global__ __launch_bounds__(ADA_T) void k_cnn_adasum_apply(float* __restrict__ params, uint16_t* __restrict__ frag,
                                                            XgmiView xv, CnnSegEnds segs,
                                                            const double* __restrict__ gram) {
  constexpr int NG = NR * (NR + 1) / 2;
  __shared__ double s_G[NR * NR];
  __shared__ double s_w[NR];
  __shared__ float s_wf[NR];
  __shared__ uint32_t s_state[2];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid == 0) {  // one read per workgroup: every thread takes the same branch
    s_state[0] = __hip_atomic_load(xv.state + kXgmiStateError, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_state[1] = __hip_atomic_load(xv.state + kXgmiStateEpoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (s_state[0] != 0u) return;
  const uint32_t epoch = s_state[1];
  const int p = b * ADA_T + tid;
  const int lo = b * ADA_T;
  const int hi = lo + ADA_T < NPARAM ? lo + ADA_T : NPARAM;
  int s = 0;
  while (s < ADA_NSEG - 1 && segs.end[s] <= lo) ++s;
  for (int plo = lo; plo < hi && s < ADA_NSEG; ++s) {
    const int phi = segs.end[s] < hi ? segs.end[s] : hi;
    const int seg_lo = s == 0 ? 0 : segs.end[s - 1];
    const int row0 = seg_lo / ADA_T + s, row1 = (segs.end[s] - 1) / ADA_T + s;
    if (tid < NG) {
      double t = gram[static_cast<int64_t>(row0) * kXgmiGramRow + tid];
      for (int row = row0 + 1; row <= row1; ++row) t += gram[static_cast<int64_t>(row) * kXgmiGramRow + tid];
      int i = 0, k = tid;  // packed upper-triangle index -> (i, j)
      while (k >= NR - i) {
        k -= NR - i;
        ++i;
      }
      const int j = i + k;
      s_G[i * NR + j] = t;
      s_G[j * NR + i] = t;
    }
    __syncthreads();
    if (tid == 0) {
      adasum_weights(s_G, NR, s_w);
      for (int r = 0; r < NR; ++r) s_wf[r] = static_cast<float>(s_w[r]);
    }
    __syncthreads();
    if (p >= plo && p < phi) {
      float acc = s_wf[0] * xgmi_slot(xv, 0, epoch)[p];
#pragma unroll
      for (int r = 1; r < NR; ++r) acc = __fmaf_rn(s_wf[r], xgmi_slot(xv, r, epoch)[p], acc);
      const float w = params[p] + acc;
      params[p] = w;
      write_frag(frag, p, w);
    }
    plo = phi;
  }
}

hipError_t cnn_adasum_step(float* params, const float* grads, void* frag, const CnnUpdate& u, const XgmiView& xv,
                           double* gram, int gram_rows, hipStream_t s) {
  // cnn_opt_fused's rules, plus the step words every mode's ticket uses here
  if (!cnn_update_valid(u) || u.hp == nullptr || u.step == nullptr || (reinterpret_cast<uintptr_t>(frag) & 15))
    return hipErrorInvalidValue;
  // a power-of-two world (the Adasum tree), one flag row and one staging float per parameter for each workgroup,
  // Gram row b + s inside the workspace
  if (xv.size < 2 || xv.size > kXgmiMaxRanks || (xv.size & (xv.size - 1)) != 0 || xv.rank < 0 || xv.rank >= xv.size)
    return hipErrorInvalidValue;
  if (xv.blocks < ADA_BLOCKS || xv.slot_bytes < static_cast<int64_t>(NPARAM) * 4 || gram == nullptr ||
      gram_rows < ADA_BLOCKS + ADA_NSEG)
    return hipErrorInvalidValue;
  using DeltaFn = decltype(&k_cnn_adasum_delta<0, 2>);
  using ApplyFn = decltype(&k_cnn_adasum_apply<2>);
  static const DeltaFn kDelta[3][4] = {
      {&k_cnn_adasum_delta<0, 2>, &k_cnn_adasum_delta<1, 2>, &k_cnn_adasum_delta<2, 2>, &k_cnn_adasum_delta<3, 2>},
      {&k_cnn_adasum_delta<0, 4>, &k_cnn_adasum_delta<1, 4>, &k_cnn_adasum_delta<2, 4>, &k_cnn_adasum_delta<3, 4>},
      {&k_cnn_adasum_delta<0, 8>, &k_cnn_adasum_delta<1, 8>, &k_cnn_adasum_delta<2, 8>, &k_cnn_adasum_delta<3, 8>}};
  static const ApplyFn kApply[3] = {&k_cnn_adasum_apply<2>, &k_cnn_adasum_apply<4>, &k_cnn_adasum_apply<8>};
  const int wi = xv.size == 2 ? 0 : xv.size == 4 ? 1 : 2;
  hipLaunchKernelGGL(kDelta[wi][u.mode], dim3(ADA_BLOCKS), dim3(ADA_T), 0, s, params, grads, u.m, u.v, u.hp, u.step,
                     xv, kCnnSegEnds, gram);
  hipLaunchKernelGGL(kApply[wi], dim3(ADA_BLOCKS), dim3(ADA_T), 0, s, params, static_cast<uint16_t*>(frag), xv,
                     kCnnSegEnds, gram);
  return hipGetLastError();
}

}  // namespace pde
