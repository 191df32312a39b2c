// FP8 linear-layer kernels (csrc/kernels/gemm_fp8.hip): the NT GEMM on v_mfma_f32_16x16x128_f8f6f4 with its four
// epilogues, the table-driven quantiser and the scale update.  OCP e4m3 (max 448) and e5m2 (max 57344).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pde {

enum Fp8Format : int { kE4M3 = 0, kE5M2 = 1 };  // the MFMA's cbsz / blgp operand-format codes
enum Fp8Epilogue : int { kFp8F32 = 0, kFp8FwdQ = 1, kFp8DgradQ = 2, kFp8Wgrad = 3 };

inline float fp8_max(int fmt) { return fmt == kE4M3 ? 448.f : 57344.f; }

// Per-tensor scale record, four floats in device memory: q = fp8(clamp(x * scale)), x ~= q * inv_scale; amax is the
// running max |x| of the step as the bit pattern of a non-negative float (integer atomicMax: order-independent);
// fmax is the format's largest finite value.
struct Fp8Rec {
  float scale, inv_scale, amax, fmax;
};

// C[M][N] = sum_k A[M][k] * B[N][k]: both operands FP8 bytes, K contiguous, the same byte pitch Kp (a multiple of 128,
// padding bytes 0x00), 16-byte aligned; fp32 accumulation; descaled by recA.inv_scale * recB.inv_scale.
// M <= 2^20 (its tiles are the grid's y dimension); a larger M is hipErrorInvalidValue.
//   kFp8F32:    out[m * ldo + n] = C (+ bias[n]), fp32.
//   kFp8FwdQ:   y = relu(C + bias[n]); q[m][n] and qt[n][m] = e4m3(clamp(y * recO.scale)); recO.amax |= max y.
//               q rows are ldq bytes and written up to the N tile's end with zeros (ldq a multiple of 64 >= N);
//               qt rows are ldqt bytes (a multiple of 64 >= M), columns m >= M written as zeros.
//   kFp8DgradQ: as kFp8FwdQ without bias and ReLU, zeroed where mask[m * ldmask + n] is a zero byte, to e5m2.
//   kFp8Wgrad:  out[m * ldo + n] = (or +=, accumulate) C; gbias[m] = (or +=) sum_k A[m][k] * recA.inv_scale if given
//               (one more MFMA per k-step against a fragment of ones, by the workgroups of N tile 0).
struct Fp8GemmArgs {
  const uint8_t *A, *B;
  int M, N, Kp;
  const Fp8Rec *recA, *recB;
  Fp8Rec* recO;
  const float* bias;
  const uint8_t* mask;
  int ldmask;
  uint8_t *q, *qt;
  int ldq, ldqt;
  float* out;
  int ldo;
  float* gbias;
  int accumulate;
};
hipError_t fp8_gemm(int afmt, int bfmt, int epi, const Fp8GemmArgs& a, hipStream_t s);

// One tensor of a quantiser launch: src [rows][cols] fp32 or bf16 with row pitch lds (elements); dst [rows][ldd] and,
// if dstT, dstT [cols][ldt] FP8 bytes (ldd a multiple of 64 >= cols, ldt a multiple of 64 >= rows, 16-byte aligned;
// padding written as zeros); rec: index of its scale record.
struct Fp8QuantEntry {
  const void* src;
  uint8_t *dst, *dstT;
  int rows, cols, lds, ldd, ldt, rec, bf16, pad;
};
// tab: n entries in device memory; blocks_x workgroups per entry walk its 64x64 tiles.
hipError_t fp8_quant(int fmt, const Fp8QuantEntry* tab, int n, int blocks_x, Fp8Rec* recs, hipStream_t s);
// One tensor, its entry passed as a kernel argument: nothing is kept between calls, the source may move.
hipError_t fp8_quant_one(int fmt, const Fp8QuantEntry& e, Fp8Rec* recs, hipStream_t s);

// For each of n records: scale = 2^floor(log2(fmax / amax)) (unchanged if amax is 0 or not finite), amax = 0.
hipError_t fp8_scales(Fp8Rec* recs, int n, hipStream_t s);

}  // namespace pde
