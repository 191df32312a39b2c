// Trust-ratio optimisers (gfx950): LAMB (Adam with a per-tensor trust ratio) and LARS (SGD with one) over ALL
// parameter tensors of a group in TWO ordinary launches on the optimiser's OptimEntry / OptimChunk table.
//
// The ratio of a tensor needs two L2 norms over the WHOLE tensor before one element of it can move, and a tensor
// spans many chunks (blocks).  Instead of a grid barrier the step is cut at the kernel boundary:
//
//   k_trust_norms  walks the chunks block-stride, software-pipelined (the next chunk's 16-byte loads are in flight
//                  during this chunk's math).  LAMB: m and v are updated in registers and stored, u is formed, and
//                  the chunk's sum p^2 / sum u^2 are reduced.  LARS: sum p^2 / sum g'^2, nothing else stored.
//                  Reduction order is fixed: a thread's 16 elements in index order, the wave's xor butterfly, the
//                  four waves through LDS summed by one thread in wave order.  ONE 8-byte store: norms[chunk].
//   k_trust_apply  one block per chunk.  Every wave sums norms[c0 .. c0 + nc) of the chunk's tensor (TrustSpan):
//                  lane i takes entries i, i + 64, ..., then the same butterfly -- every chunk of a tensor derives
//                  the bitwise same ratio whatever the scheduling.  LAMB reloads p, m, v (not g), recomputes u with
//                  the operations of launch 1 (lamb_u below, every operation spelled out) and applies it; LARS reloads
//                  p, g, m, forms d and updates m and p.  p, the state and the bf16 compute copy are stored; the
//                  last block to arrive publishes the step count through the {steps taken, arrival} ticket.
//
// No atomics on data, no spin, no wait on another workgroup, no co-residency: a workgroup that is not resident
// runs later.  Both launches are hipGraph-capturable; hyper-parameters and the step count are read from device
// memory.  Accesses: the 16-byte / scalar split of ChunkRegs (OptimEntry::vec, chunk tails) and the non-temporal
// policy of optim.hip.  Summing a tensor's chunk norms costs nc / 64 loads per lane per block: nothing for the
// models here (the largest tensor is 500 chunks), quadratic for a tensor of many millions of chunks.
#include <cstdlib>

#include "optim_device.h"

namespace pde {

namespace {

using optdev::bias_correction;
using optdev::kOptChunk;
using optdev::kOptGroups;
using optdev::kOptThreads;
using optdev::ld4;
using optdev::st4;

constexpr int kWaves = kOptThreads / 64;

struct TrustHyper {
  float lr, b1, b2, omb1, omb2, eps, wd, mom, gscale, trust, inv_bc1, inv_sqrt_bc2;
  int step;
};

// KIND 0 LAMB, 1 LARS.  LARS keeps its trust coefficient in the slot of beta1 (HP_TRUST), which it has no use for.
template <int KIND>
__device__ __forceinline__ TrustHyper load_trust_hyper(const float* __restrict__ hp, int step) {
  TrustHyper h;
  h.lr = hp[HP_LR]; h.eps = hp[HP_EPS]; h.wd = hp[HP_WD]; h.gscale = hp[HP_GRAD_SCALE];
  h.b1 = hp[HP_BETA1]; h.b2 = hp[HP_BETA2]; h.omb1 = hp[HP_OMB1]; h.omb2 = hp[HP_OMB2];
  h.mom = hp[HP_MOMENTUM]; h.trust = hp[HP_TRUST];
  h.step = step;
  h.inv_bc1 = 1.f;
  h.inv_sqrt_bc2 = 1.f;
  if (KIND == 0) {
    h.inv_bc1 = __fdiv_rn(1.f, bias_correction(h.omb1, step));
    h.inv_sqrt_bc2 = rsqrtf(bias_correction(h.omb2, step));
  }
  return h;
}

// LAMB's u = (m / bc1) / (sqrt(v / bc2) + eps) + wd p.  Launch 1 takes its norm and launch 2 applies it: one
// spelled-out sequence, so both see the same bits.
__device__ __forceinline__ float lamb_u(const TrustHyper& h, float p, float m, float v) {
  const float r = __fdiv_rn(__fmul_rn(m, h.inv_bc1), fmaf(sqrtf(v), h.inv_sqrt_bc2, h.eps));
  return fmaf(h.wd, p, r);
}

// One chunk's share of NA state tensors for one thread: kOptGroups x 16 B of each, all loads issued before any
// math.  A null source reads as zeros.
template <int NA, int NT>
struct TrustRegs {
  float a[NA][kOptGroups][4];
  int e0[kOptGroups], cnt[kOptGroups];
  int tensor, vec;

  __device__ __forceinline__ void load(const OptimChunk& ch, int vec_, const float* const (&src)[NA]) {
    tensor = ch.tensor;
    vec = vec_;
    const int end = ch.start + ch.count;
#pragma unroll
    for (int u = 0; u < kOptGroups; ++u) {
      e0[u] = ch.start + (u * kOptThreads + threadIdx.x) * 4;
      cnt[u] = e0[u] < end ? min(4, end - e0[u]) : 0;
#pragma unroll
      for (int s = 0; s < NA; ++s) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a[s][u][k] = 0.f;
        if (src[s] == nullptr) continue;
        if (cnt[u] == 4 && vec) {
          const f32x4 x = ld4<NT>(src[s] + e0[u]);
          a[s][u][0] = x[0]; a[s][u][1] = x[1]; a[s][u][2] = x[2]; a[s][u][3] = x[3];
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < cnt[u]) a[s][u][k] = src[s][e0[u] + k];
        }
      }
    }
  }

  __device__ __forceinline__ void store(int s, float* dst) const {
#pragma unroll
    for (int u = 0; u < kOptGroups; ++u) {
      if (cnt[u] == 4 && vec) {
        st4<NT>(dst + e0[u], f32x4{a[s][u][0], a[s][u][1], a[s][u][2], a[s][u][3]});
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < cnt[u]) dst[e0[u] + k] = a[s][u][k];
      }
    }
  }

  __device__ __forceinline__ void store_bf16(int s, uint16_t* dst) const {
#pragma unroll
    for (int u = 0; u < kOptGroups; ++u) {
      if (cnt[u] == 4 && vec) {
        st_vec(reinterpret_cast<u16x4*>(dst + e0[u]),
               u16x4{f2bf(a[s][u][0]), f2bf(a[s][u][1]), f2bf(a[s][u][2]), f2bf(a[s][u][3])}, NT == 2);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < cnt[u]) dst[e0[u] + k] = f2bf(a[s][u][k]);
      }
    }
  }
};

// Launch 1.  Arrays -- LAMB: 0 p, 1 g, 2 m, 3 v; LARS: 0 p, 1 g.
template <int KIND, int NT>
__global__ __launch_bounds__(kOptThreads) void k_trust_norms(const OptimEntry* __restrict__ tab,
                                                             const OptimChunk* __restrict__ chunks, int nchunks,
                                                             const float* __restrict__ hp,
                                                             const int* __restrict__ step_ptr,
                                                             float2* __restrict__ norms) {
  constexpr int NA = KIND == 0 ? 4 : 2;
  __shared__ float s_part[2][kWaves][2];  // two sets: one barrier per chunk
  const TrustHyper h = load_trust_hyper<KIND>(hp, step_ptr[0] + 1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int stride = static_cast<int>(gridDim.x);
  TrustRegs<NA, NT> cur, nxt;

  auto issue = [&](TrustRegs<NA, NT>& r, int c) {
    const OptimChunk ch = chunks[c];
    const OptimEntry& te = tab[ch.tensor];
    if constexpr (KIND == 0) {
      const float* const src[NA] = {te.param, te.grad, te.exp_avg, te.exp_avg_sq};
      r.load(ch, te.vec, src);
    } else {
      const float* const src[NA] = {te.param, te.grad};
      r.load(ch, te.vec, src);
    }
  };

  int c = static_cast<int>(blockIdx.x);
  if (c < nchunks) issue(cur, c);
  int set = 0;
  for (; c < nchunks; c += stride) {
    if (c + stride < nchunks) issue(nxt, c + stride);
    float sp = 0.f, sq = 0.f;  // sum p^2, sum u^2 (LAMB) / sum g'^2 (LARS): zero-filled tail elements add nothing
#pragma unroll
    for (int u = 0; u < kOptGroups; ++u) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k >= cur.cnt[u]) continue;
        const float p = cur.a[0][u][k];
        const float g = __fmul_rn(cur.a[1][u][k], h.gscale);
        sp = fmaf(p, p, sp);
        if constexpr (KIND == 0) {
          const float m = fmaf(h.b1, cur.a[2][u][k], __fmul_rn(h.omb1, g));
          const float v = fmaf(h.b2, cur.a[3][u][k], __fmul_rn(__fmul_rn(h.omb2, g), g));
          cur.a[2][u][k] = m;
          cur.a[3][u][k] = v;
          const float uu = lamb_u(h, p, m, v);
          sq = fmaf(uu, uu, sq);
        } else {
          sq = fmaf(g, g, sq);
        }
      }
    }
    if constexpr (KIND == 0) {
      const OptimEntry& te = tab[cur.tensor];
      cur.store(2, te.exp_avg);
      cur.store(3, te.exp_avg_sq);
    }
    sp = wave_sum(sp);
    sq = wave_sum(sq);
    if (lane == 0) {
      s_part[set][wave][0] = sp;
      s_part[set][wave][1] = sq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float a = s_part[set][0][0], b = s_part[set][0][1];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        a = __fadd_rn(a, s_part[set][w][0]);
        b = __fadd_rn(b, s_part[set][w][1]);
      }
      norms[c] = make_float2(a, b);
    }
    set ^= 1;
    cur = nxt;
  }
}

// Launch 2, one block per chunk.  Arrays -- LAMB: 0 p, 1 m, 2 v; LARS: 0 p, 1 g, 2 m.
template <int KIND, int NT>
__global__ __launch_bounds__(kOptThreads) void k_trust_apply(const OptimEntry* __restrict__ tab,
                                                             const OptimChunk* __restrict__ chunks,
                                                             const TrustSpan* __restrict__ spans,
                                                             const float2* __restrict__ norms,
                                                             const float* __restrict__ hp, int* __restrict__ step_ptr) {
  __shared__ int s_step;
  if (threadIdx.x == 0) s_step = step_ptr[0] + 1;  // step being taken (1-based)
  __syncthreads();
  const TrustHyper h = load_trust_hyper<KIND>(hp, s_step);
  const bool use_m = KIND == 0 || h.mom != 0.f;
  const OptimChunk ch = chunks[blockIdx.x];
  const OptimEntry& te = tab[ch.tensor];
  const TrustSpan span = spans[ch.tensor];

  TrustRegs<3, NT> r;
  if constexpr (KIND == 0) {
    const float* const src[3] = {te.param, te.exp_avg, te.exp_avg_sq};
    r.load(ch, te.vec, src);
  } else {
    const float* const src[3] = {te.param, te.grad, use_m ? te.exp_avg : nullptr};
    r.load(ch, te.vec, src);
  }

  // the tensor's two squared norms: every wave of every chunk of the tensor sums the same entries in the same order
  float sp = 0.f, sq = 0.f;
  for (int i = threadIdx.x & 63; i < span.nc; i += 64) {
    const float2 n = norms[span.c0 + i];
    sp = __fadd_rn(sp, n.x);
    sq = __fadd_rn(sq, n.y);
  }
  const float pn = sqrtf(wave_sum(sp)), qn = sqrtf(wave_sum(sq));
  float ratio = 1.f;
  if (pn > 0.f && qn > 0.f) {
    if (KIND == 0) ratio = __fdiv_rn(pn, qn);
    else ratio = __fdiv_rn(__fmul_rn(h.trust, pn), __fadd_rn(fmaf(h.wd, pn, qn), h.eps));
  }
  const float lamb_step = __fmul_rn(h.lr, ratio);

#pragma unroll
  for (int u = 0; u < kOptGroups; ++u) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= r.cnt[u]) continue;
      const float p = r.a[0][u][k];
      if constexpr (KIND == 0) {
        r.a[0][u][k] = fmaf(-lamb_step, lamb_u(h, p, r.a[1][u][k], r.a[2][u][k]), p);
      } else {
        const float g = __fmul_rn(r.a[1][u][k], h.gscale);
        float d = __fmul_rn(ratio, fmaf(h.wd, p, g));
        if (use_m) {
          d = (h.step == 1) ? d : fmaf(h.mom, r.a[2][u][k], d);
          r.a[2][u][k] = d;
        }
        r.a[0][u][k] = fmaf(-h.lr, d, p);
      }
    }
  }
  r.store(0, te.param);
  if (KIND == 1 && use_m) r.store(2, te.exp_avg);
  if (te.bf16_copy) r.store_bf16(0, te.bf16_copy);

  // The last block to arrive publishes the new step count (the ticket of run_chunks: every block consumed the
  // old count before the barrier above, the next launch sees the store across the kernel boundary).
  __syncthreads();
  if (threadIdx.x == 0) {
    const int prev = atomicAdd(step_ptr + 1, 1);
    if (prev == static_cast<int>(gridDim.x) - 1) {
      step_ptr[0] = s_step;
      step_ptr[1] = 0;
    }
  }
}

template <int KIND, int NT>
void launch_trust(const OptimEntry* tab, const OptimChunk* chunks, int nchunks, const TrustSpan* spans, float2* norms,
                  const float* hp, int* step, hipStream_t s) {
  hipLaunchKernelGGL((k_trust_norms<KIND, NT>), dim3(static_cast<unsigned>(optim_segment_blocks(nchunks))),
                     dim3(kOptThreads), 0, s, tab, chunks, nchunks, hp, step, norms);
  hipLaunchKernelGGL((k_trust_apply<KIND, NT>), dim3(static_cast<unsigned>(nchunks)), dim3(kOptThreads), 0, s, tab,
                     chunks, spans, norms, hp, step);
}

}  // namespace

hipError_t multi_tensor_trust(int kind, const OptimEntry* dev_table, const OptimChunk* dev_chunks, int nchunks,
                              const TrustSpan* dev_spans, float* dev_norms, const float* dev_hparams, int* dev_step,
                              hipStream_t s) {
  if ((kind != 0 && kind != 1) || nchunks < 0 || !dev_table || !dev_chunks || !dev_spans || !dev_norms ||
      !dev_hparams || !dev_step)
    return hipErrorInvalidValue;
  if (nchunks == 0) return hipSuccess;
  // the size rule of multi_tensor_optim_range (PDE_OPTIM_NT overrides it there and here)
  static const int nt_env = std::getenv("PDE_OPTIM_NT") ? std::atoi(std::getenv("PDE_OPTIM_NT")) : -1;
  const int nt = nt_env >= 0 ? nt_env : (static_cast<long>(nchunks) * kOptChunk >= (8L << 20) ? 1 : 0);
  float2* norms = reinterpret_cast<float2*>(dev_norms);
#define PDE_TRUST(K)                                                                                    \
  if (nt == 2) launch_trust<K, 2>(dev_table, dev_chunks, nchunks, dev_spans, norms, dev_hparams, dev_step, s);      \
  else if (nt == 1) launch_trust<K, 1>(dev_table, dev_chunks, nchunks, dev_spans, norms, dev_hparams, dev_step, s); \
  else launch_trust<K, 0>(dev_table, dev_chunks, nchunks, dev_spans, norms, dev_hparams, dev_step, s);
  if (kind == 0) {
    PDE_TRUST(0)
  } else {
    PDE_TRUST(1)
  }
#undef PDE_TRUST
  return hipGetLastError();
}

}  // namespace pde
