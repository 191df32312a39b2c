// One-shot peer all-reduce over xGMI: see xgmi_allreduce.h for the protocol.
#include <hip/hip_runtime.h>

#include <chrono>
#include <deque>
#include <mutex>
#include <thread>
#include <utility>
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "adasum_weights.h"
#include "xgmi_allreduce.h"
#include "xgmi_device.h"

namespace pde {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ uint16_t bf16_bits(float f) {  // round to nearest even
  const uint32_t u = __float_as_uint(f);
  return static_cast<uint16_t>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float bf16_float(uint16_t b) { return __uint_as_float(static_cast<uint32_t>(b) << 16); }

void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("xgmi allreduce: ") + what + ": " + hipGetErrorString(e));
}

// grid = one workgroup per chunk of `chunk` elements (the same grid on every rank for the same n: workgroup
// b waits for the peers' flags of workgroup b).  The epoch is per call (xgmi_epoch), not per workgroup.
// WIRE_BF16: the staged chunk is bf16 (cast fused into the staging store, half the bytes over xGMI); the
// rank-order sum is fp32 either way.
template <int NR, bool VEC, bool WIRE_BF16>
__global__ __launch_bounds__(kThreads) void k_xgmi_oneshot(const float* src, float* dst, int64_t n, float scale,
                                                            XgmiView xv, int64_t chunk) {
  __shared__ uint32_t s_epoch;
  __shared__ int s_fail;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const uint32_t epoch = xgmi_epoch(xv, b, &s_epoch);
  const int64_t lo = static_cast<int64_t>(b) * chunk;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  float* mine = xgmi_slot(xv, xv.rank, epoch);

  // 1. stage this workgroup's chunk into my exported slot
  if constexpr (WIRE_BF16) {
    uint16_t* mine16 = reinterpret_cast<uint16_t*>(mine);
    if (VEC) {
      for (int64_t i = lo + 4 * tid; i < hi; i += 4 * kThreads) {
        const float4 v = *reinterpret_cast<const float4*>(src + i);
        *reinterpret_cast<ushort4*>(mine16 + i) = make_ushort4(bf16_bits(v.x), bf16_bits(v.y), bf16_bits(v.z),
                                                               bf16_bits(v.w));
      }
    } else {
      for (int64_t i = lo + tid; i < hi; i += kThreads) mine16[i] = bf16_bits(src[i]);
    }
  } else if (VEC) {
    for (int64_t i = lo + 4 * tid; i < hi; i += 4 * kThreads)
      *reinterpret_cast<float4*>(mine + i) = *reinterpret_cast<const float4*>(src + i);
  } else {
    for (int64_t i = lo + tid; i < hi; i += kThreads) mine[i] = src[i];
  }
  // 2.-3. publish my chunk to every peer and wait for theirs
  if (xgmi_publish_and_wait(xv, b, epoch, &s_fail)) {
    xgmi_read_delay(xv);
    // 4. sum the chunk over all ranks' slots in rank order (bit-identical on every rank)
    if constexpr (WIRE_BF16) {
      const uint16_t* s16[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) s16[r] = reinterpret_cast<const uint16_t*>(xgmi_slot(xv, r, epoch));
      if (VEC) {
        for (int64_t i = lo + 4 * tid; i < hi; i += 4 * kThreads) {
          ushort4 u[NR];
#pragma unroll
          for (int r = 0; r < NR; ++r) u[r] = *reinterpret_cast<const ushort4*>(s16[r] + i);
          float4 acc = make_float4(bf16_float(u[0].x), bf16_float(u[0].y), bf16_float(u[0].z), bf16_float(u[0].w));
#pragma unroll
          for (int r = 1; r < NR; ++r) {
            acc.x += bf16_float(u[r].x);
            acc.y += bf16_float(u[r].y);
            acc.z += bf16_float(u[r].z);
            acc.w += bf16_float(u[r].w);
          }
          *reinterpret_cast<float4*>(dst + i) = make_float4(acc.x * scale, acc.y * scale, acc.z * scale, acc.w * scale);
        }
      } else {
        for (int64_t i = lo + tid; i < hi; i += kThreads) {
          float acc = bf16_float(s16[0][i]);
#pragma unroll
          for (int r = 1; r < NR; ++r) acc += bf16_float(s16[r][i]);
          dst[i] = acc * scale;
        }
      }
      xgmi_finish(xv, b, epoch);
      return;
    }
    const float* slots[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) slots[r] = xgmi_slot(xv, r, epoch);
    if (VEC) {
      for (int64_t i = lo + 4 * tid; i < hi; i += 4 * kThreads) {
        float4 v[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) v[r] = *reinterpret_cast<const float4*>(slots[r] + i);
        float4 acc = v[0];
#pragma unroll
        for (int r = 1; r < NR; ++r) {
          acc.x += v[r].x;
          acc.y += v[r].y;
          acc.z += v[r].z;
          acc.w += v[r].w;
        }
        acc.x *= scale;
        acc.y *= scale;
        acc.z *= scale;
        acc.w *= scale;
        *reinterpret_cast<float4*>(dst + i) = acc;
      }
    } else {
      for (int64_t i = lo + tid; i < hi; i += kThreads) {
        float v[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) v[r] = slots[r][i];
        float acc = v[0];
#pragma unroll
        for (int r = 1; r < NR; ++r) acc += v[r];
        dst[i] = acc * scale;
      }
    }
  }
  // 5. this workgroup's epoch advances
  xgmi_finish(xv, b, epoch);
}

// ---- two-shot: reduce-scatter + all-gather, for bandwidth-bound buckets ------------------------------------
// The bucket is cut into NR rank-chunks of `cn` elements and every rank-chunk into gridDim.x pieces of `pc`
// elements.  Workgroup b of every rank owns piece b of all NR rank-chunks:
//   1. stages its pieces of its own bucket into its slot (bf16 wire: cast fused into the store), raises flag 2e-1
//      in every rank's flag array and waits for the peers' 2e-1 (all NR pieces b are staged everywhere);
//   2. reduces piece b of MY rank-chunk over all NR slots in rank order (the only reader of that range of my slot
//      in this call is me), scales it and stores the sum in place in my slot and in dst;
//   3. raises flag 2e, waits for the peers' 2e and copies piece b of every OTHER rank-chunk -- its owner's sum --
//      from that owner's slot into dst.
// Each link carries 2/NR of the bucket (the one-shot: all of it), every element is summed by exactly one rank and
// read back by the others, so the result is bit-identical everywhere; with a bf16 wire the owner keeps the
// bf16-rounded sum too.  Flags rise monotonically (2e-1, 2e per call, e = the instance's call epoch), so an
// instance runs two-shot calls only (XgmiAllreduce::allreduce_twoshot refuses a mix with one-shot calls).
template <bool WIRE_BF16>
struct Wire;
template <>
struct Wire<false> {
  using T = float;
  using V = float4;
  __device__ static float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }
  __device__ static void store4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
  __device__ static float4 round4(float4 v) { return v; }
  __device__ static float get(const float* p) { return *p; }
  __device__ static void put(float* p, float v) { *p = v; }
  __device__ static float round1(float v) { return v; }
};
template <>
struct Wire<true> {
  using T = uint16_t;
  __device__ static float4 load4(const uint16_t* p) {
    const ushort4 u = *reinterpret_cast<const ushort4*>(p);
    return make_float4(bf16_float(u.x), bf16_float(u.y), bf16_float(u.z), bf16_float(u.w));
  }
  __device__ static void store4(uint16_t* p, float4 v) {
    *reinterpret_cast<ushort4*>(p) = make_ushort4(bf16_bits(v.x), bf16_bits(v.y), bf16_bits(v.z), bf16_bits(v.w));
  }
  __device__ static float4 round4(float4 v) {
    return make_float4(bf16_float(bf16_bits(v.x)), bf16_float(bf16_bits(v.y)), bf16_float(bf16_bits(v.z)),
                       bf16_float(bf16_bits(v.w)));
  }
  __device__ static float get(const uint16_t* p) { return bf16_float(*p); }
  __device__ static void put(uint16_t* p, float v) { *p = bf16_bits(v); }
  __device__ static float round1(float v) { return bf16_float(bf16_bits(v)); }
};

template <int NR, bool VEC, bool WIRE_BF16>
__global__ __launch_bounds__(kThreads) void k_xgmi_twoshot(const float* src, float* dst, int64_t n, float scale,
                                                            XgmiView xv, int64_t cn, int64_t pc) {
  using W = Wire<WIRE_BF16>;
  using T = typename W::T;
  __shared__ uint32_t s_epoch;
  __shared__ int s_fail;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const uint32_t epoch = xgmi_epoch(xv, b, &s_epoch);
  const int me = xv.rank;
  auto range = [&](int q, int64_t& lo, int64_t& hi) {
    const int64_t c0 = static_cast<int64_t>(q) * cn, c1 = c0 + cn < n ? c0 + cn : n;
    lo = c0 + static_cast<int64_t>(b) * pc;
    hi = lo + pc < c1 ? lo + pc : c1;
  };
  T* mine = reinterpret_cast<T*>(xgmi_slot(xv, me, epoch));
  // 1. stage my pieces b of all rank-chunks
#pragma unroll
  for (int q = 0; q < NR; ++q) {
    int64_t lo, hi;
    range(q, lo, hi);
    if (VEC) {
      for (int64_t i = lo + 4 * tid; i < hi; i += 4 * kThreads) W::store4(mine + i, *reinterpret_cast<const float4*>(src + i));
    } else {
      for (int64_t i = lo + tid; i < hi; i += kThreads) W::put(mine + i, src[i]);
    }
  }
  if (!xgmi_publish_and_wait(xv, b, 2u * epoch - 1u, &s_fail)) {
    xgmi_finish(xv, b, epoch);
    return;
  }
  xgmi_read_delay(xv);
  // 2. reduce piece b of my rank-chunk (rank order), keep the sum in my slot for the peers
  {
    const T* slots[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) slots[r] = reinterpret_cast<const T*>(xgmi_slot(xv, r, epoch));
    int64_t lo, hi;
    range(me, lo, hi);
    if (VEC) {
      for (int64_t i = lo + 4 * tid; i < hi; i += 4 * kThreads) {
        float4 v[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) v[r] = W::load4(slots[r] + i);
        float4 acc = v[0];
#pragma unroll
        for (int r = 1; r < NR; ++r) {
          acc.x += v[r].x;
          acc.y += v[r].y;
          acc.z += v[r].z;
          acc.w += v[r].w;
        }
        acc = W::round4(make_float4(acc.x * scale, acc.y * scale, acc.z * scale, acc.w * scale));
        W::store4(mine + i, acc);
        *reinterpret_cast<float4*>(dst + i) = acc;
      }
    } else {
      for (int64_t i = lo + tid; i < hi; i += kThreads) {
        float v[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) v[r] = W::get(slots[r] + i);
        float acc = v[0];
#pragma unroll
        for (int r = 1; r < NR; ++r) acc += v[r];
        acc = W::round1(acc * scale);
        W::put(mine + i, acc);
        dst[i] = acc;
      }
    }
  }
  // 3. gather the owners' sums of the other rank-chunks
  if (xgmi_publish_and_wait(xv, b, 2u * epoch, &s_fail)) {
#pragma unroll
    for (int d = 1; d < NR; ++d) {
      const int q = (me + d) % NR;  // start at a different owner on every rank: the links load evenly
      const T* theirs = reinterpret_cast<const T*>(xgmi_slot(xv, q, epoch));
      int64_t lo, hi;
      range(q, lo, hi);
      if (VEC) {
        for (int64_t i = lo + 4 * tid; i < hi; i += 4 * kThreads)
          *reinterpret_cast<float4*>(dst + i) = W::load4(theirs + i);
      } else {
        for (int64_t i = lo + tid; i < hi; i += kThreads) dst[i] = W::get(theirs + i);
      }
    }
  }
  xgmi_finish(xv, b, epoch);
}

template <int NR, bool W>
void launch2_w(bool vec, dim3 grid, hipStream_t s, const float* src, float* dst, int64_t n, float scale,
               const XgmiView& v, int64_t cn, int64_t pc) {
  if (vec)
    hipLaunchKernelGGL((k_xgmi_twoshot<NR, true, W>), grid, dim3(kThreads), 0, s, src, dst, n, scale, v, cn, pc);
  else
    hipLaunchKernelGGL((k_xgmi_twoshot<NR, false, W>), grid, dim3(kThreads), 0, s, src, dst, n, scale, v, cn, pc);
}
template <int NR>
void launch2(bool vec, bool wire_bf16, dim3 grid, hipStream_t s, const float* src, float* dst, int64_t n, float scale,
             const XgmiView& v, int64_t cn, int64_t pc) {
  if (wire_bf16)
    launch2_w<NR, true>(vec, grid, s, src, dst, n, scale, v, cn, pc);
  else
    launch2_w<NR, false>(vec, grid, s, src, dst, n, scale, v, cn, pc);
}

__global__ void k_scale(const float* src, float* dst, int64_t n, float scale) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x)
    dst[i] = src[i] * scale;
}

// ---- Adasum: Gram pass (with the peer exchange) + weights and combine --------------------------------------
// adasum_weights.h: the Adasum tree of N rank vectors is sum_r w_r x_r with the w_r a function of the Gram matrix
// G[i][j] = x_i . x_j alone -- per TENSOR (segment) of the fused buffer.  Both launches use the one-shot grid (one
// workgroup per chunk, the same on every rank).  A PIECE is (segment s) x (chunk b); its partial Gram goes to
// workspace row b + s: consecutive pieces advance b, s or both, so the row is unique, rows of one segment are
// contiguous, and the last one is < blocks + kMaxAdasumSegs.
constexpr int kGramMax = kXgmiMaxRanks * (kXgmiMaxRanks + 1) / 2;  // workspace row: packed upper triangle, <= 36
static_assert(kGramMax == kXgmiGramRow, "the row pitch kernels outside this file use (xgmi_view.h)");
constexpr int kWaves = kThreads / 64;

struct AdasumSegs {
  int count;
  int64_t end[kMaxAdasumSegs];  // cumulative element ends; end[count - 1] == n
};

// [plo, phi) as a scalar head up to the next multiple of 4, a float4 body and a scalar tail: the split depends on
// the indices alone (the slots are 4 KB aligned), so every rank walks a piece in the same order.
#define PDE_PIECE_SPLIT(plo, phi)                                                      \
  const int64_t a_lo = ((plo) + 3) / 4 * 4 < (phi) ? ((plo) + 3) / 4 * 4 : (phi);      \
  const int64_t a_hi = (phi) / 4 * 4 > a_lo ? (phi) / 4 * 4 : a_lo

// Launch 1.  VEC: the staging copy runs in float4 (src 16-byte aligned, n % 4 == 0); the slot reads do not depend
// on it.  Products of fp32 values are exact in fp64 and the sums are fp64, reduced in a fixed order (per-thread
// stride, wave shuffle, the workgroup's waves in order): no floating-point atomics, the same bits on every rank.
template <int NR, bool VEC>
__global__ __launch_bounds__(kThreads) void k_xgmi_adasum_gram(const float* src, int64_t n, XgmiView xv, int64_t chunk,
                                                                AdasumSegs segs, double* gram) {
  constexpr int NG = NR * (NR + 1) / 2;
  __shared__ uint32_t s_epoch;
  __shared__ int s_fail;
  __shared__ double s_part[kWaves][NG];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const uint32_t epoch = xgmi_epoch(xv, b, &s_epoch);
  const int64_t lo = static_cast<int64_t>(b) * chunk;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  float* mine = xgmi_slot(xv, xv.rank, epoch);
  if (VEC) {
    for (int64_t i = lo + 4 * tid; i < hi; i += 4 * kThreads)
      *reinterpret_cast<float4*>(mine + i) = *reinterpret_cast<const float4*>(src + i);
  } else {
    for (int64_t i = lo + tid; i < hi; i += kThreads) mine[i] = src[i];
  }
  if (xgmi_publish_and_wait(xv, b, epoch, &s_fail)) {
    xgmi_read_delay(xv);
    const float* slots[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) slots[r] = xgmi_slot(xv, r, epoch);
    int s = 0;
    while (s < segs.count - 1 && segs.end[s] <= lo) ++s;  // the first segment that reaches into this chunk
    for (int64_t plo = lo; plo < hi && s < segs.count; ++s) {
      const int64_t phi = segs.end[s] < hi ? segs.end[s] : hi;
      double g[NG];
#pragma unroll
      for (int k = 0; k < NG; ++k) g[k] = 0.0;
      auto add = [&](const float (&x)[NR]) {
        int k = 0;
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
          for (int j = i; j < NR; ++j) g[k++] += static_cast<double>(x[i]) * static_cast<double>(x[j]);
      };
      auto add1 = [&](int64_t i) {
        float x[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) x[r] = slots[r][i];
        add(x);
      };
      PDE_PIECE_SPLIT(plo, phi);
      for (int64_t i = plo + tid; i < a_lo; i += kThreads) add1(i);
      for (int64_t i = a_lo + 4 * tid; i < a_hi; i += 4 * kThreads) {
        float4 v[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) v[r] = *reinterpret_cast<const float4*>(slots[r] + i);
        float x[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) x[r] = v[r].x;
        add(x);
#pragma unroll
        for (int r = 0; r < NR; ++r) x[r] = v[r].y;
        add(x);
#pragma unroll
        for (int r = 0; r < NR; ++r) x[r] = v[r].z;
        add(x);
#pragma unroll
        for (int r = 0; r < NR; ++r) x[r] = v[r].w;
        add(x);
      }
      for (int64_t i = a_hi + tid; i < phi; i += kThreads) add1(i);
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
        for (int w = 1; w < kWaves; ++w) t += s_part[w][tid];
        gram[static_cast<int64_t>(b + s) * kGramMax + tid] = t;
      }
      __syncthreads();  // s_part is reused by the next piece
      plo = phi;
    }
  }
  xgmi_finish(xv, b, epoch);
}

// Launch 2.  It RE-READS the peers' slots of the call launch 1 exchanged (no N-fold local copy).  They still hold
// this call's bytes: a peer overwrites slot (e & 1) only in its call e + 2, which starts only after its call e + 1
// saw this rank's flags of e + 1, i.e. after this rank launched call e + 1 -- and on this stream call e + 1 starts
// behind this launch (the argument of xgmi_device.h, one launch further).  The epoch is the one launch 1's
// xgmi_finish just stored.  A set error word (a timed-out or aborted wait, in this call or an earlier one not yet
// cleared) means some chunk's Gram or bytes are missing: nothing is written, as the sum path drops its result.
// Every workgroup sums the partial rows of the segments it touches in row order and derives the weights with the
// same code from the same bits, on every rank; dst = scale * sum_r (float)w_r * slot_r[i] in rank order with
// explicit fmas, so the scalar and float4 forms (VEC: dst 16-byte aligned) give the same bits too.
template <int NR, bool VEC>
__global__ __launch_bounds__(kThreads) void k_xgmi_adasum_combine(float* dst, int64_t n, float scale, XgmiView xv,
                                                                   int64_t chunk, AdasumSegs segs, const double* gram) {
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
  const int64_t lo = static_cast<int64_t>(b) * chunk;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  const float* slots[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) slots[r] = xgmi_slot(xv, r, epoch);
  int s = 0;
  while (s < segs.count - 1 && segs.end[s] <= lo) ++s;
  for (int64_t plo = lo; plo < hi && s < segs.count; ++s) {
    const int64_t phi = segs.end[s] < hi ? segs.end[s] : hi;
    const int64_t seg_lo = s == 0 ? 0 : segs.end[s - 1];
    const int64_t row0 = seg_lo / chunk + s, row1 = (segs.end[s] - 1) / chunk + s;
    if (tid < NG) {
      double t = gram[row0 * kGramMax + tid];
      for (int64_t row = row0 + 1; row <= row1; ++row) t += gram[row * kGramMax + tid];
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
    float w[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) w[r] = s_wf[r];
    auto one = [&](int64_t i) {
      float x[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) x[r] = slots[r][i];
      float acc = w[0] * x[0];
#pragma unroll
      for (int r = 1; r < NR; ++r) acc = __fmaf_rn(w[r], x[r], acc);
      dst[i] = acc * scale;
    };
    if (VEC) {
      PDE_PIECE_SPLIT(plo, phi);
      for (int64_t i = plo + tid; i < a_lo; i += kThreads) one(i);
      for (int64_t i = a_lo + 4 * tid; i < a_hi; i += 4 * kThreads) {
        float4 v[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) v[r] = *reinterpret_cast<const float4*>(slots[r] + i);
        float4 acc = make_float4(w[0] * v[0].x, w[0] * v[0].y, w[0] * v[0].z, w[0] * v[0].w);
#pragma unroll
        for (int r = 1; r < NR; ++r) {
          acc.x = __fmaf_rn(w[r], v[r].x, acc.x);
          acc.y = __fmaf_rn(w[r], v[r].y, acc.y);
          acc.z = __fmaf_rn(w[r], v[r].z, acc.z);
          acc.w = __fmaf_rn(w[r], v[r].w, acc.w);
        }
        *reinterpret_cast<float4*>(dst + i) = make_float4(acc.x * scale, acc.y * scale, acc.z * scale, acc.w * scale);
      }
      for (int64_t i = a_hi + tid; i < phi; i += kThreads) one(i);
    } else {
      for (int64_t i = plo + tid; i < phi; i += kThreads) one(i);
    }
    plo = phi;
  }
}
#undef PDE_PIECE_SPLIT

template <int NR>
void launch_adasum(bool vec_src, bool vec_dst, dim3 grid, hipStream_t s, const float* src, float* dst, int64_t n,
                   float scale, const XgmiView& v, int64_t chunk, const AdasumSegs& segs, double* gram) {
  if (vec_src)
    hipLaunchKernelGGL((k_xgmi_adasum_gram<NR, true>), grid, dim3(kThreads), 0, s, src, n, v, chunk, segs, gram);
  else
    hipLaunchKernelGGL((k_xgmi_adasum_gram<NR, false>), grid, dim3(kThreads), 0, s, src, n, v, chunk, segs, gram);
  if (vec_dst)
    hipLaunchKernelGGL((k_xgmi_adasum_combine<NR, true>), grid, dim3(kThreads), 0, s, dst, n, scale, v, chunk, segs,
                       gram);
  else
    hipLaunchKernelGGL((k_xgmi_adasum_combine<NR, false>), grid, dim3(kThreads), 0, s, dst, n, scale, v, chunk, segs,
                       gram);
}

template <int NR, bool W>
void launch_w(bool vec, dim3 grid, hipStream_t s, const float* src, float* dst, int64_t n, float scale,
              const XgmiView& v, int64_t chunk) {
  if (vec)
    hipLaunchKernelGGL((k_xgmi_oneshot<NR, true, W>), grid, dim3(kThreads), 0, s, src, dst, n, scale, v, chunk);
  else
    hipLaunchKernelGGL((k_xgmi_oneshot<NR, false, W>), grid, dim3(kThreads), 0, s, src, dst, n, scale, v, chunk);
}
template <int NR>
void launch(bool vec, bool wire_bf16, dim3 grid, hipStream_t s, const float* src, float* dst, int64_t n, float scale,
            const XgmiView& v, int64_t chunk) {
  if (wire_bf16)
    launch_w<NR, true>(vec, grid, s, src, dst, n, scale, v, chunk);
  else
    launch_w<NR, false>(vec, grid, s, src, dst, n, scale, v, chunk);
}

}  // namespace

XgmiAllreduce::XgmiAllreduce(int rank, int size, int device, int64_t max_bytes, int blocks, double timeout_s)
    : rank_(rank), size_(size), device_(device), blocks_(blocks), max_bytes_(max_bytes) {
  if (size < 1 || size > kXgmiMaxRanks) throw std::invalid_argument("xgmi allreduce: 1..8 ranks");
  if (blocks < 1 || blocks > 1024) throw std::invalid_argument("xgmi allreduce: 1..1024 workgroups");
  slot_bytes_ = ((max_bytes + 4095) / 4096) * 4096;
  flag_bytes_ = ((static_cast<int64_t>(blocks) * kXgmiMaxRanks * 4 + 4095) / 4096) * 4096;
  timeout_ticks_ = static_cast<uint64_t>(timeout_s * 1e8);  // s_memrealtime runs at 100 MHz
  hip_check(hipSetDevice(device), "hipSetDevice");
  const size_t bytes = static_cast<size_t>(flag_bytes_ + 2 * slot_bytes_);
  void* p = nullptr;
  hip_check(hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached), "hipExtMallocWithFlags(uncached)");
  local_ = static_cast<char*>(p);
  hip_check(hipMemset(local_, 0, bytes), "zero flags");
  void* st = nullptr;
  hip_check(hipMalloc(&st, kXgmiStateWords * 4), "hipMalloc state");
  state_ = static_cast<uint32_t*>(st);
  hip_check(hipMemset(state_, 0, kXgmiStateWords * 4), "zero state");
  void* hp = nullptr;
  hip_check(hipHostMalloc(&hp, kXgmiHostWords * 4, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc");
  host_ = static_cast<uint32_t*>(hp);
  std::memset(host_, 0, kXgmiHostWords * 4);
  void* hd = nullptr;
  hip_check(hipHostGetDevicePointer(&hd, hp, 0), "hipHostGetDevicePointer");
  host_dev_ = static_cast<uint32_t*>(hd);
  if (size > 1) {  // adasum's partial-Gram rows, sized once: never allocated during a (captured) call
    const size_t gb = static_cast<size_t>(blocks + kMaxAdasumSegs) * kGramMax * sizeof(double);
    void* gp = nullptr;
    hip_check(hipMalloc(&gp, gb), "hipMalloc gram workspace");
    gram_ = static_cast<double*>(gp);
    hip_check(hipMemset(gram_, 0, gb), "zero gram workspace");
  }
  hip_check(hipDeviceSynchronize(), "sync after init");  // flags are zero before any peer can map them
  peers_.assign(size, nullptr);
  peers_[rank] = local_;
}

XgmiAllreduce::~XgmiAllreduce() {
  try {
    close();
  } catch (...) {
  }
}

std::string XgmiAllreduce::ipc_handle() const {
  hipIpcMemHandle_t h;
  // (a few spaced attempts before giving up -- a host call, no GPU work; the "invalid argument" seen with several
  // processes sharing one card right after a close did not clear this way: see tests/test_xgmi_twoshot_gpu.py)
  hipError_t e = hipErrorUnknown;
  for (int attempt = 0; attempt < 4; ++attempt) {
    e = hipIpcGetMemHandle(&h, local_);
    if (e == hipSuccess) break;
    (void)hipGetLastError();
    std::this_thread::sleep_for(std::chrono::milliseconds(50 * (attempt + 1)));
  }
  hip_check(e, "hipIpcGetMemHandle");
  return std::string(reinterpret_cast<const char*>(&h), sizeof(h));
}

void XgmiAllreduce::open(const std::vector<std::string>& handles) {
  if (static_cast<int>(handles.size()) != size_) throw std::invalid_argument("xgmi allreduce: one handle per rank");
  hip_check(hipSetDevice(device_), "hipSetDevice");
  for (int r = 0; r < size_; ++r) {
    if (r == rank_) continue;
    if (handles[r].size() != sizeof(hipIpcMemHandle_t)) throw std::invalid_argument("xgmi allreduce: bad handle");
    hipIpcMemHandle_t h;
    std::memcpy(&h, handles[r].data(), sizeof(h));
    void* p = nullptr;
    hip_check(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess), "hipIpcOpenMemHandle");
    peers_[r] = static_cast<char*>(p);
  }
  opened_ = true;
}

void XgmiAllreduce::allreduce(const float* src, float* dst, int64_t n, float scale, hipStream_t s,
                              bool wire_bf16) {
  if (n <= 0) return;
  if (n * 4 > max_bytes_) throw std::invalid_argument("xgmi allreduce: bucket exceeds max_bytes");
  if (mode_ == 2) throw std::logic_error("xgmi allreduce: an instance runs one-shot OR two-shot calls, not both");
  mode_ = 1;
  if (size_ == 1) {
    const int g = static_cast<int>(std::min<int64_t>(1024, (n + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(k_scale, dim3(g), dim3(kThreads), 0, s, src, dst, n, scale);
    hip_check(hipGetLastError(), "scale launch");
    return;
  }
  if (!opened_) throw std::runtime_error("xgmi allreduce: peers not opened");
  const XgmiView v = view();
  // chunk per workgroup: >= 1 KB (small buckets use few workgroups: each one pays a flag round trip), a
  // multiple of 64 floats (256 B rows) so float4 lanes stay aligned; grid <= blocks_
  int64_t chunk = std::max<int64_t>((n + blocks_ - 1) / blocks_, 256);
  chunk = ((chunk + 63) / 64) * 64;
  const bool vec = (n % 4 == 0) && (reinterpret_cast<uintptr_t>(src) % 16 == 0) &&
                   (reinterpret_cast<uintptr_t>(dst) % 16 == 0);
  const dim3 grid(static_cast<unsigned>((n + chunk - 1) / chunk));
  switch (size_) {
    case 2: launch<2>(vec, wire_bf16, grid, s, src, dst, n, scale, v, chunk); break;
    case 3: launch<3>(vec, wire_bf16, grid, s, src, dst, n, scale, v, chunk); break;
    case 4: launch<4>(vec, wire_bf16, grid, s, src, dst, n, scale, v, chunk); break;
    case 5: launch<5>(vec, wire_bf16, grid, s, src, dst, n, scale, v, chunk); break;
    case 6: launch<6>(vec, wire_bf16, grid, s, src, dst, n, scale, v, chunk); break;
    case 7: launch<7>(vec, wire_bf16, grid, s, src, dst, n, scale, v, chunk); break;
    default: launch<8>(vec, wire_bf16, grid, s, src, dst, n, scale, v, chunk); break;
  }
  hip_check(hipGetLastError(), "oneshot launch");
  ++calls_;
}

void XgmiAllreduce::allreduce_twoshot(const float* src, float* dst, int64_t n, float scale, hipStream_t s,
                                      bool wire_bf16) {
  if (n <= 0) return;
  if (n * 4 > max_bytes_) throw std::invalid_argument("xgmi allreduce: bucket exceeds max_bytes");
  if (mode_ == 1) throw std::logic_error("xgmi allreduce: an instance runs one-shot OR two-shot calls, not both");
  mode_ = 2;
  if (size_ == 1) {
    const int g = static_cast<int>(std::min<int64_t>(1024, (n + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(k_scale, dim3(g), dim3(kThreads), 0, s, src, dst, n, scale);
    hip_check(hipGetLastError(), "scale launch");
    return;
  }
  if (!opened_) throw std::runtime_error("xgmi allreduce: peers not opened");
  const XgmiView v = view();
  // rank-chunks and pieces are multiples of 64 floats (float4 lanes stay aligned); >= 1024 elements per piece
  // (a piece pays two flag round trips), at most blocks_ pieces per rank-chunk
  int64_t cn = (n + size_ - 1) / size_;
  cn = ((cn + 63) / 64) * 64;
  int64_t pc = std::max<int64_t>((cn + blocks_ - 1) / blocks_, 1024);
  pc = ((pc + 63) / 64) * 64;
  const dim3 grid(static_cast<unsigned>((cn + pc - 1) / pc));
  const bool vec = (n % 4 == 0) && (reinterpret_cast<uintptr_t>(src) % 16 == 0) &&
                   (reinterpret_cast<uintptr_t>(dst) % 16 == 0);
  switch (size_) {
    case 2: launch2<2>(vec, wire_bf16, grid, s, src, dst, n, scale, v, cn, pc); break;
    case 3: launch2<3>(vec, wire_bf16, grid, s, src, dst, n, scale, v, cn, pc); break;
    case 4: launch2<4>(vec, wire_bf16, grid, s, src, dst, n, scale, v, cn, pc); break;
    case 5: launch2<5>(vec, wire_bf16, grid, s, src, dst, n, scale, v, cn, pc); break;
    case 6: launch2<6>(vec, wire_bf16, grid, s, src, dst, n, scale, v, cn, pc); break;
    case 7: launch2<7>(vec, wire_bf16, grid, s, src, dst, n, scale, v, cn, pc); break;
    default: launch2<8>(vec, wire_bf16, grid, s, src, dst, n, scale, v, cn, pc); break;
  }
  hip_check(hipGetLastError(), "twoshot launch");
  ++calls_;
}

void XgmiAllreduce::adasum(const float* src, float* dst, int64_t n, const std::vector<int64_t>& segs, float scale,
                           hipStream_t s) {
  if (n <= 0) return;
  if (n * 4 > max_bytes_) throw std::invalid_argument("xgmi adasum: bucket exceeds max_bytes");
  if (mode_ == 2) throw std::logic_error("xgmi adasum: runs on a one-shot instance, not a two-shot one");
  if ((size_ & (size_ - 1)) != 0) throw std::invalid_argument("xgmi adasum: the world size must be a power of two");
  if (segs.empty() || static_cast<int>(segs.size()) > kMaxAdasumSegs)
    throw std::invalid_argument("xgmi adasum: 1.." + std::to_string(kMaxAdasumSegs) + " segments per call");
  AdasumSegs tab{};
  tab.count = static_cast<int>(segs.size());
  int64_t end = 0;
  for (int i = 0; i < tab.count; ++i) {
    if (segs[i] <= 0) throw std::invalid_argument("xgmi adasum: empty segment");
    end += segs[i];
    tab.end[i] = end;
  }
  if (end != n) throw std::invalid_argument("xgmi adasum: segment lengths do not sum to the element count");
  mode_ = 1;
  if (size_ == 1) {
    const int g = static_cast<int>(std::min<int64_t>(1024, (n + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(k_scale, dim3(g), dim3(kThreads), 0, s, src, dst, n, scale);
    hip_check(hipGetLastError(), "scale launch");
    return;
  }
  if (!opened_) throw std::runtime_error("xgmi allreduce: peers not opened");
  const XgmiView v = view();
  // the one-shot grid (allreduce above): the same chunks on every rank
  int64_t chunk = std::max<int64_t>((n + blocks_ - 1) / blocks_, 256);
  chunk = ((chunk + 63) / 64) * 64;
  const dim3 grid(static_cast<unsigned>((n + chunk - 1) / chunk));
  const bool vec_src = (n % 4 == 0) && (reinterpret_cast<uintptr_t>(src) % 16 == 0);
  const bool vec_dst = reinterpret_cast<uintptr_t>(dst) % 16 == 0;
  switch (size_) {
    case 2: launch_adasum<2>(vec_src, vec_dst, grid, s, src, dst, n, scale, v, chunk, tab, gram_); break;
    case 4: launch_adasum<4>(vec_src, vec_dst, grid, s, src, dst, n, scale, v, chunk, tab, gram_); break;
    default: launch_adasum<8>(vec_src, vec_dst, grid, s, src, dst, n, scale, v, chunk, tab, gram_); break;
  }
  hip_check(hipGetLastError(), "adasum launch");
  ++calls_;
}

XgmiView XgmiAllreduce::view() const {
  if (size_ > 1 && !opened_) throw std::runtime_error("xgmi allreduce: peers not opened");
  XgmiView v{};
  for (int r = 0; r < size_; ++r) v.base[r] = peers_[r];
  v.state = state_;
  v.host = host_dev_;
  v.timeout_ticks = timeout_ticks_;
  v.read_delay_ticks = read_delay_ticks_;
  v.flag_bytes = flag_bytes_;
  v.slot_bytes = slot_bytes_;
  v.rank = rank_;
  v.size = size_;
  v.blocks = blocks_;
  return v;
}

int XgmiAllreduce::error(bool sync) {
  if (host_ == nullptr) return 0;
  if (sync) {
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipDeviceSynchronize(), "sync");
  }
  return __atomic_load_n(host_ + kXgmiHostError, __ATOMIC_ACQUIRE) != 0u ? 1 : 0;
}

void XgmiAllreduce::clear_error() {
  if (host_ == nullptr) return;
  hip_check(hipSetDevice(device_), "hipSetDevice");
  hip_check(hipDeviceSynchronize(), "sync");
  hip_check(hipMemset(state_ + kXgmiStateError, 0, 4), "clear error word");
  hip_check(hipDeviceSynchronize(), "sync");
  __atomic_store_n(host_ + kXgmiHostError, 0u, __ATOMIC_RELEASE);
}

void XgmiAllreduce::abort() {
  if (host_ != nullptr) __atomic_store_n(host_ + kXgmiHostAbort, 1u, __ATOMIC_RELEASE);
}

void XgmiAllreduce::reset_abort() {
  if (host_ != nullptr) __atomic_store_n(host_ + kXgmiHostAbort, 0u, __ATOMIC_RELEASE);
}

bool XgmiAllreduce::aborted() const {
  return host_ != nullptr && __atomic_load_n(host_ + kXgmiHostAbort, __ATOMIC_ACQUIRE) != 0u;
}

namespace {
// Exported slot buffers of closed instances, freed only a few closes later: a peer may still have the buffer
// mapped when this rank closes (the ranks close one after another, with no barrier -- a failure path must not
// wait for dead peers), so a new instance allocated right away must not reuse the range while that stale mapping
// is alive.  A precaution: the intermittent hipIpcGetMemHandle "invalid argument" seen with 4 processes sharing
// one card after a close (tests/test_xgmi_twoshot_gpu.py) persisted with it.  At most kRetired buffers stay.
constexpr size_t kRetired = 4;
std::mutex g_retired_mu;
std::deque<std::pair<int, void*>> g_retired;  // (device, buffer)
void retire(int device, void* p) {
  std::lock_guard<std::mutex> lk(g_retired_mu);
  g_retired.emplace_back(device, p);
  while (g_retired.size() > kRetired) {
    (void)hipSetDevice(g_retired.front().first);
    (void)hipFree(g_retired.front().second);
    g_retired.pop_front();
  }
  (void)hipSetDevice(device);
}
}  // namespace

void XgmiAllreduce::close() {
  if (local_ == nullptr) return;
  (void)hipSetDevice(device_);
  (void)hipDeviceSynchronize();
  for (int r = 0; r < size_; ++r)
    if (r != rank_ && peers_[r] != nullptr) (void)hipIpcCloseMemHandle(peers_[r]);
  peers_.clear();
  retire(device_, local_);
  (void)hipFree(state_);
  if (gram_ != nullptr) (void)hipFree(gram_);
  gram_ = nullptr;
  if (host_ != nullptr) (void)hipHostFree(host_);
  local_ = nullptr;
  state_ = nullptr;
  host_ = host_dev_ = nullptr;
  opened_ = false;
}

}  // namespace pde
