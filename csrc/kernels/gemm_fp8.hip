// FP8 linear layers for gfx950: one NT GEMM on v_mfma_f32_16x16x128_f8f6f4 (k_gemm_fp8) with the forward, data-
// gradient and weight-gradient epilogues fused, the table-driven quantiser (k_fp8_quant) and the per-tensor scale
// update (k_fp8_scales).  Contract: csrc/include/gemm_fp8.h.
//
// k_gemm_fp8: a workgroup of 4 waves owns a BM x 64 output tile (BM = 64, or 32 when 64 would leave half the chip
// idle -- the quantising epilogues need the whole K sum in one place, so small batches get more tiles from a shorter
// M tile, not from split-K).  One k-step is 128 bytes of K: a single MFMA per 16x16 sub-tile.  A wave owns 16 of the
// tile's 64 columns and all BM rows, so per k-step it reads one B fragment and BM/16 A fragments from LDS and issues
// BM/16 MFMAs.  Fragment map of the 128-wide instruction: lane l holds row (l & 15), k bytes [32 * (l >> 4), +32) --
// two 16-byte LDS reads.  LDS rows are 144 bytes (128 + 16): row r starts at dword 36 r, and 36 r mod 64 takes the 16
// values 0, 4, .., 60 once each over 16 rows, so the 16 lanes of a k-group cover all 64 banks exactly once per read.
// Global -> LDS: 16-byte loads, 8 threads a row, the next k-step's loads issued before the current k-step's MFMAs and
// stored into the other LDS buffer after them (one barrier per k-step).  Rows past M / N are loaded as zeros; the K
// padding of the operands is zero bytes in memory.
#include "gemm_fp8.h"

#include "common.cuh"

namespace pde {

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kBN = 64, kBK = 128, kPitch = kBK + 16, kThreads = 256, kStagePitch = 80;
constexpr int kUnitScale = 0x7f7f7f7f;  // E8M0 2^0 in every byte: the MFMA's block scales are not used

template <int AF, int BF>
__device__ __forceinline__ f32x4 mfma128(const i32x8& a, const i32x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, AF, BF, 0, kUnitScale, 0, kUnitScale);
}

__device__ __forceinline__ i32x8 lds_frag(const uint8_t* p) {
  const i32x4 lo = *reinterpret_cast<const i32x4*>(p), hi = *reinterpret_cast<const i32x4*>(p + 16);
  return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// four floats -> four FP8 bytes (byte j = value j): clamp to the format's finite range, round to nearest even
template <int FMT>
__device__ __forceinline__ uint32_t quant4(float a, float b, float c, float d, float scale) {
  constexpr float mx = FMT == kE4M3 ? 448.f : 57344.f;
  a = fminf(fmaxf(a * scale, -mx), mx);
  b = fminf(fmaxf(b * scale, -mx), mx);
  c = fminf(fmaxf(c * scale, -mx), mx);
  d = fminf(fmaxf(d * scale, -mx), mx);
  int v = 0;
  if constexpr (FMT == kE4M3) {
    v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, v, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
  } else {
    v = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, v, false);
    v = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, v, true);
  }
  return static_cast<uint32_t>(v);
}

// running maximum of a non-negative float as an integer atomicMax on its bit pattern (order-independent)
__device__ __forceinline__ void fold_amax(Fp8Rec* rec, float v) {
  atomicMax(reinterpret_cast<unsigned int*>(&rec->amax), __float_as_uint(v));
}

template <int AF, int BF, int EPI, int BM>
__global__ __launch_bounds__(kThreads) void k_gemm_fp8(const Fp8GemmArgs p) {
  constexpr int MT = BM / 16, AP = BM / 32, BP = kBN / 32, kBuf = (BM + kBN) * kPitch;
  static_assert(BM == 32 || BM == 64, "M tile");
  static_assert(BM * kStagePitch <= 2 * kBuf, "the epilogue's staging tile reuses the operand buffers");
  __shared__ __attribute__((aligned(16))) uint8_t smem[2 * kBuf];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * kBN, m0 = blockIdx.y * BM;
  const int lr = tid >> 3, lc = (tid & 7) * 16;  // this thread's row and byte column of a 32-row load pass
  const int nk = p.Kp / kBK;

  i32x4 ra[AP], rb[BP];
  auto gload = [&](int ks) {
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      const int row = m0 + lr + 32 * i;
      ra[i] = row < p.M ? *reinterpret_cast<const i32x4*>(p.A + static_cast<long>(row) * p.Kp + ks * kBK + lc)
                        : i32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < BP; ++i) {
      const int row = n0 + lr + 32 * i;
      rb[i] = row < p.N ? *reinterpret_cast<const i32x4*>(p.B + static_cast<long>(row) * p.Kp + ks * kBK + lc)
                        : i32x4{0, 0, 0, 0};
    }
  };
  auto sstore = [&](int buf) {
    uint8_t* sa = smem + buf * kBuf;
    uint8_t* sb = sa + BM * kPitch;
#pragma unroll
    for (int i = 0; i < AP; ++i) *reinterpret_cast<i32x4*>(sa + (lr + 32 * i) * kPitch + lc) = ra[i];
#pragma unroll
    for (int i = 0; i < BP; ++i) *reinterpret_cast<i32x4*>(sb + (lr + 32 * i) * kPitch + lc) = rb[i];
  };

  f32x4 acc[MT], bacc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) acc[i] = bacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  // bias gradient = row sums of A: one more MFMA per k-step against ones (0x38 = 1.0 in e4m3), wave 0 of N tile 0
  const bool rowsum = EPI == kFp8Wgrad && p.gbias != nullptr && blockIdx.x == 0 && wave == 0;
  constexpr int k1 = 0x38383838;
  const i32x8 ones{k1, k1, k1, k1, k1, k1, k1, k1};

  gload(0);
  sstore(0);
  __syncthreads();
  for (int ks = 0; ks < nk; ++ks) {
    if (ks + 1 < nk) gload(ks + 1);
    const uint8_t* sa = smem + (ks & 1) * kBuf;
    const uint8_t* sb = sa + BM * kPitch;
    const i32x8 bf = lds_frag(sb + (16 * wave + c) * kPitch + 32 * g);
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const i32x8 af = lds_frag(sa + (16 * i + c) * kPitch + 32 * g);
      acc[i] = mfma128<AF, BF>(af, bf, acc[i]);
      if constexpr (EPI == kFp8Wgrad)
        if (rowsum) bacc[i] = mfma128<AF, kE4M3>(af, ones, bacc[i]);
    }
    if (ks + 1 < nk) sstore((ks + 1) & 1);
    __syncthreads();  // buffer (ks + 1) & 1 written, buffer ks & 1 read by every wave
  }

  // lane (c, g) holds C[16 i + 4 g + r][16 wave + c] in acc[i][r]
  const float inv_a = p.recA->inv_scale, descale = inv_a * p.recB->inv_scale;
  const int n = n0 + 16 * wave + c;
  if constexpr (EPI == kFp8F32 || EPI == kFp8Wgrad) {
    const float bias = (EPI == kFp8F32 && p.bias != nullptr && n < p.N) ? p.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + 16 * i + 4 * g + r;
        if (m >= p.M) continue;
        if (n < p.N) {
          float* o = p.out + static_cast<long>(m) * p.ldo + n;
          const float v = acc[i][r] * descale + bias;
          *o = (EPI == kFp8Wgrad && p.accumulate) ? *o + v : v;
        }
        if constexpr (EPI == kFp8Wgrad)
          if (rowsum && c == 0) {
            const float v = bacc[i][r] * inv_a;
            p.gbias[m] = p.accumulate ? p.gbias[m] + v : v;
          }
      }
  } else {
    constexpr int QF = EPI == kFp8FwdQ ? kE4M3 : kE5M2;
    const float scale = p.recO->scale;
    const float bias = (EPI == kFp8FwdQ && n < p.N) ? p.bias[n] : 0.f;
    uint8_t* st = smem;  // [BM][kStagePitch] bytes: the row-major copy leaves as 16-byte row chunks
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      float y[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + 16 * i + 4 * g + r;
        const bool valid = m < p.M && n < p.N;
        float v = acc[i][r] * descale;
        if constexpr (EPI == kFp8FwdQ) {
          v = fmaxf(v + bias, 0.f);
        } else {  // the producer's ReLU mask: its quantised activation is +-0
          if (valid && (p.mask[static_cast<long>(m) * p.ldmask + n] & 0x7f) == 0) v = 0.f;
        }
        y[r] = valid ? v : 0.f;
        amax = fmaxf(amax, fabsf(y[r]));
      }
      const uint32_t w = quant4<QF>(y[0], y[1], y[2], y[3], scale);
      // transposed copy: the lane's four rows are four consecutive bytes of row n
      if (n < p.N) *reinterpret_cast<uint32_t*>(p.qt + static_cast<long>(n) * p.ldqt + m0 + 16 * i + 4 * g) = w;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        st[(16 * i + 4 * g + r) * kStagePitch + 16 * wave + c] = static_cast<uint8_t>(w >> (8 * r));
    }
    __syncthreads();
    for (int id = tid; id < BM * 4; id += kThreads) {
      const int row = id >> 2, cq = (id & 3) * 16;
      if (m0 + row < p.M && n0 + cq + 16 <= p.ldq)
        *reinterpret_cast<i32x4*>(p.q + static_cast<long>(m0 + row) * p.ldq + n0 + cq) =
            *reinterpret_cast<const i32x4*>(st + row * kStagePitch + cq);
    }
    amax = wave_max(amax);
    if (lane == 0) fold_amax(p.recO, amax);
  }
}

template <int AF, int BF, int EPI>
hipError_t launch_gemm(const Fp8GemmArgs& a, hipStream_t s) {
  const long tiles64 = static_cast<long>(ceil_div(a.M, 64)) * ceil_div(a.N, kBN);
  if (tiles64 >= 128) {
    hipLaunchKernelGGL((k_gemm_fp8<AF, BF, EPI, 64>), dim3(ceil_div(a.N, kBN), ceil_div(a.M, 64)), dim3(kThreads), 0, s,
                       a);
  } else {
    hipLaunchKernelGGL((k_gemm_fp8<AF, BF, EPI, 32>), dim3(ceil_div(a.N, kBN), ceil_div(a.M, 32)), dim3(kThreads), 0, s,
                       a);
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Quantiser: a workgroup walks 64x64 tiles of one table entry; a thread converts 16 consecutive columns of a row
// (one 16-byte store), the tile passes through LDS for the transposed copy (16 consecutive rows of a column).
// ------------------------------------------------------------------------------------------------
template <int FMT>
__global__ __launch_bounds__(kThreads) void k_fp8_quant(const Fp8QuantEntry* __restrict__ tab, Fp8Rec* recs,
                                                       const Fp8QuantEntry one) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[64 * kStagePitch];
  __shared__ float red[kThreads / 64];
  // a single tensor travels as a kernel argument (its address may change from call to call: no table to rebuild)
  const Fp8QuantEntry e = tab != nullptr ? tab[blockIdx.y] : one;
  const float scale = recs[e.rec].scale;
  const int tid = threadIdx.x, r = tid >> 2, cq = (tid & 3) * 16;
  const int tc = e.ldd / 64, nt = (e.rows + 63) / 64 * tc;
  const bool vec = e.lds % 8 == 0 && (reinterpret_cast<uintptr_t>(e.src) & 15) == 0;
  float amax = 0.f;
  for (int t = blockIdx.x; t < nt; t += gridDim.x) {
    const int r0 = (t / tc) * 64, c0 = (t % tc) * 64, row = r0 + r, col = c0 + cq;
    float v[16];
    if (row < e.rows && col + 16 <= e.cols && vec) {
      if (e.bf16) {
        const u16x8* s = reinterpret_cast<const u16x8*>(static_cast<const uint16_t*>(e.src) +
                                                        static_cast<long>(row) * e.lds + col);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const u16x8 x = s[j];
#pragma unroll
          for (int k = 0; k < 8; ++k) v[8 * j + k] = bf2f(x[k]);
        }
      } else {
        const f32x4* s = reinterpret_cast<const f32x4*>(static_cast<const float*>(e.src) +
                                                        static_cast<long>(row) * e.lds + col);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 x = s[j];
#pragma unroll
          for (int k = 0; k < 4; ++k) v[4 * j + k] = x[k];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const bool in = row < e.rows && col + j < e.cols;
        const long at = static_cast<long>(row) * e.lds + col + j;
        v[j] = !in ? 0.f : e.bf16 ? bf2f(static_cast<const uint16_t*>(e.src)[at]) : static_cast<const float*>(e.src)[at];
      }
    }
    u32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[j] = quant4<FMT>(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3], scale);
#pragma unroll
      for (int k = 0; k < 4; ++k) amax = fmaxf(amax, fabsf(v[4 * j + k]));
    }
    if (row < e.rows) *reinterpret_cast<u32x4*>(e.dst + static_cast<long>(row) * e.ldd + col) = w;
    if (e.dstT != nullptr) {  // uniform over the workgroup
      *reinterpret_cast<u32x4*>(tile + r * kStagePitch + cq) = w;
      __syncthreads();
      u32x4 wt{0u, 0u, 0u, 0u};  // column r of the tile, rows cq .. cq + 15
#pragma unroll
      for (int j = 0; j < 16; ++j) wt[j >> 2] |= static_cast<uint32_t>(tile[(cq + j) * kStagePitch + r]) << (8 * (j & 3));
      if (c0 + r < e.cols) *reinterpret_cast<u32x4*>(e.dstT + static_cast<long>(c0 + r) * e.ldt + r0 + cq) = wt;
      __syncthreads();
    }
  }
  amax = wave_max(amax);
  if ((tid & 63) == 0) red[tid >> 6] = amax;
  __syncthreads();
  if (tid == 0) fold_amax(&recs[e.rec], fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
}

__global__ void k_fp8_scales(Fp8Rec* recs, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float a = recs[i].amax;
  if (a > 0.f && a < INFINITY) {
    const float q = recs[i].fmax / a;
    int e = q < INFINITY ? ilogbf(q) : 126;  // floor(log2 q), exact
    e = e < -126 ? -126 : e > 126 ? 126 : e;
    recs[i].scale = ldexpf(1.f, e);
    recs[i].inv_scale = ldexpf(1.f, -e);
  }
  recs[i].amax = 0.f;
}

}  // namespace

hipError_t fp8_gemm(int afmt, int bfmt, int epi, const Fp8GemmArgs& a, hipStream_t s) {
  if (a.M < 1 || a.M > (1 << 20) || a.N < 1 || a.Kp < kBK || a.Kp % kBK != 0 || bfmt != kE4M3) return hipErrorInvalidValue;
  if (afmt == kE4M3 && epi == kFp8F32) return launch_gemm<kE4M3, kE4M3, kFp8F32>(a, s);
  if (afmt == kE4M3 && epi == kFp8FwdQ) return launch_gemm<kE4M3, kE4M3, kFp8FwdQ>(a, s);
  if (afmt == kE5M2 && epi == kFp8F32) return launch_gemm<kE5M2, kE4M3, kFp8F32>(a, s);
  if (afmt == kE5M2 && epi == kFp8DgradQ) return launch_gemm<kE5M2, kE4M3, kFp8DgradQ>(a, s);
  if (afmt == kE5M2 && epi == kFp8Wgrad) return launch_gemm<kE5M2, kE4M3, kFp8Wgrad>(a, s);
  return hipErrorInvalidValue;
}

hipError_t fp8_quant(int fmt, const Fp8QuantEntry* tab, int n, int blocks_x, Fp8Rec* recs, hipStream_t s) {
  if (tab == nullptr || n < 1 || blocks_x < 1) return hipErrorInvalidValue;
  if (fmt == kE4M3)
    hipLaunchKernelGGL(k_fp8_quant<kE4M3>, dim3(blocks_x, n), dim3(kThreads), 0, s, tab, recs, Fp8QuantEntry{});
  else
    hipLaunchKernelGGL(k_fp8_quant<kE5M2>, dim3(blocks_x, n), dim3(kThreads), 0, s, tab, recs, Fp8QuantEntry{});
  return hipGetLastError();
}

hipError_t fp8_quant_one(int fmt, const Fp8QuantEntry& e, Fp8Rec* recs, hipStream_t s) {
  if (e.src == nullptr || e.dst == nullptr || e.rows < 1 || e.cols < 1) return hipErrorInvalidValue;
  const long tiles = static_cast<long>((e.rows + 63) / 64) * (e.ldd / 64);
  const dim3 grid(static_cast<unsigned>(tiles < 256 ? tiles : 256));
  const Fp8QuantEntry* none = nullptr;
  if (fmt == kE4M3)
    hipLaunchKernelGGL(k_fp8_quant<kE4M3>, grid, dim3(kThreads), 0, s, none, recs, e);
  else
    hipLaunchKernelGGL(k_fp8_quant<kE5M2>, grid, dim3(kThreads), 0, s, none, recs, e);
  return hipGetLastError();
}

hipError_t fp8_scales(Fp8Rec* recs, int n, hipStream_t s) {
  if (n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fp8_scales, dim3(ceil_div(n, 64)), dim3(64), 0, s, recs, n);
  return hipGetLastError();
}

}  // namespace pde
