// Global-norm gradient clipping (gfx950) for the fused optimisers: torch.nn.utils.clip_grad_norm_ with grad_scale
// folded in, as ONE launch over the optimiser's OptimEntry / OptimChunk tables of up to kClipMaxGroups param groups.
//
// No update kernel knows about clipping.  Every one of them reads its hyper-parameters through one pointer and
// multiplies the gradient by hp[HP_GRAD_SCALE] first, so "clip, then update" is "launch the unchanged update kernel
// on a second table hp_eff whose HP_GRAD_SCALE was multiplied by the clip coefficient".  k_grad_clip produces it:
//
//   chunk walk  block-stride and software-pipelined like k_trust_norms: the next chunk's 16-byte gradient loads are
//               in flight during this chunk's squares.  Same 16-byte / scalar split (OptimEntry::vec, chunk tails),
//               same non-temporal policy NT; a null grad reads as zeros.  Reduction order is fixed: a thread's 16
//               elements in index order, the wave's xor butterfly, the four waves through LDS summed in wave order.
//               ONE 4-byte store per chunk: partials[chunk] = sum of raw g^2.
//   hand-off    the kernel's own arrival ticket in the clip workspace (not the optimiser's step words), the fenced
//               protocol of the BatchNorm finalizer (norm_pool.hip): agent-scope partial stores, drained and
//               released before the block's relaxed ticket increment; the block that draws the last ticket acquires.
//   final sum   by that last block only.  One wave per param group (wave g & 3): lane i takes the group's entries
//               i, i + 64, ..., then the butterfly; thread 0 then combines the groups in group order, each subtotal
//               weighted by its grad_scale^2 (one group: one multiply after the sqrtf), and derives coef.  The block
//               writes {total, coef} and every group's hp_eff, and clears the ticket for the next launch / replay.
//
// No spin, no wait on another workgroup, no floating-point atomics, no co-residency requirement: a workgroup that is
// not resident runs later, and whoever arrives last finishes.  max_norm is read from the workspace, so it can change
// between replays of a captured step.
#include <cstdlib>

#include "clip_device.h"
#include "optim_device.h"

namespace pde {

namespace {

using optdev::kOptChunk;
using optdev::kOptGroups;
using optdev::kOptThreads;
using optdev::ld4;

static_assert(kOptThreads == 256, "block_sum4 combines four waves");
static_assert(kClipMaxGroups == 8, "one wave takes groups w and w + 4");

// One chunk's gradient for one thread: kOptGroups x 16 B, all loads issued before any math.
template <int NT>
struct ClipRegs {
  float g[kOptGroups][4];

  __device__ __forceinline__ void load(const OptimEntry& te, const OptimChunk& ch) {
    const int end = ch.start + ch.count;
#pragma unroll
    for (int u = 0; u < kOptGroups; ++u) {
      const int e0 = ch.start + (u * kOptThreads + threadIdx.x) * 4;
      const int cnt = e0 < end ? min(4, end - e0) : 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) g[u][k] = 0.f;
      if (te.grad == nullptr) continue;
      if (cnt == 4 && te.vec) {
        const f32x4 x = ld4<NT>(te.grad + e0);
        g[u][0] = x[0]; g[u][1] = x[1]; g[u][2] = x[2]; g[u][3] = x[3];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < cnt) g[u][k] = te.grad[e0 + k];
      }
    }
  }
};

__device__ __forceinline__ void st_agent(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Lane i's share i, i + 64, ... of partials[c0, c1), eight loads per trip issued before their adds.
__device__ __forceinline__ float lane_partials(const float* part, int c0, int c1, int lane) {
  float s = 0.f;
  int i = c0 + lane;
  for (; i + 7 * 64 < c1; i += 8 * 64) {
    float u[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] = part[i + 64 * k];
#pragma unroll
    for (int k = 0; k < 8; ++k) s = __fadd_rn(s, u[k]);
  }
  for (; i < c1; i += 64) s = __fadd_rn(s, part[i]);
  return s;
}

// (G by value: every index into its arrays below is a compile-time constant, so it stays in the kernel arguments)
template <int NT>
__global__ __launch_bounds__(kOptThreads) void k_grad_clip(const ClipGroups G, int nchunks, float* ws) {
  __shared__ float s_part[2][4];  // two sets: one barrier per chunk
  __shared__ float s_grp[kClipMaxGroups];
  __shared__ float s_coef;
  __shared__ int s_last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int stride = static_cast<int>(gridDim.x);
  float* partials = ws + CLIP_PARTIALS;
  ClipRegs<NT> cur, nxt;

  auto issue = [&](ClipRegs<NT>& r, int c) {
    const OptimEntry* tab = G.tab[0];
    const OptimChunk* chunks = G.chunks[0];
    int base = 0;
#pragma unroll
    for (int i = 1; i < kClipMaxGroups; ++i) {
      if (i < G.ngroups && c >= G.c_end[i - 1]) {
        tab = G.tab[i];
        chunks = G.chunks[i];
        base = G.c_end[i - 1];
      }
    }
    const OptimChunk ch = chunks[c - base];
    r.load(tab[ch.tensor], ch);
  };

  int c = static_cast<int>(blockIdx.x);
  if (c < nchunks) issue(cur, c);
  int set = 0;
  for (; c < nchunks; c += stride) {
    if (c + stride < nchunks) issue(nxt, c + stride);
    float sq = 0.f;  // zero-filled tail elements add nothing
#pragma unroll
    for (int u = 0; u < kOptGroups; ++u) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sq = fmaf(cur.g[u][k], cur.g[u][k], sq);
    }
    const float total = clipdev::block_sum4(wave_sum(sq), s_part[set]);
    if (threadIdx.x == 0) st_agent(partials + c, total);
    set ^= 1;
    cur = nxt;
  }

  // Hand-off: thread 0 made all of this block's partial stores; they are drained and released before its ticket.
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int* ticket = reinterpret_cast<int*>(ws + CLIP_TICKET);
    const bool last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == stride - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    s_last = last;
  }
  __syncthreads();
  if (!s_last) return;

  // Final sum: group g on wave g & 3.
#pragma unroll
  for (int g = 0; g < kClipMaxGroups; ++g) {
    if (g < G.ngroups && (g & 3) == wave) {
      const float s = wave_sum(lane_partials(partials, g == 0 ? 0 : G.c_end[g - 1], G.c_end[g], lane));
      if (lane == 0) s_grp[g] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float total;
    if (G.ngroups == 1) {
      total = __fmul_rn(sqrtf(s_grp[0]), fabsf(G.hp[0][HP_GRAD_SCALE]));
    } else {
      float acc = 0.f;
#pragma unroll
      for (int g = 0; g < kClipMaxGroups; ++g) {
        if (g < G.ngroups) {
          const float gs = G.hp[g][HP_GRAD_SCALE];
          acc = fmaf(__fmul_rn(gs, gs), s_grp[g], acc);
        }
      }
      total = sqrtf(acc);
    }
    const float coef = clipdev::clip_coef(total, ws[CLIP_MAX_NORM]);
    ws[CLIP_TOTAL] = total;
    ws[CLIP_COEF] = coef;
    s_coef = coef;
    __hip_atomic_store(reinterpret_cast<int*>(ws + CLIP_TICKET), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (threadIdx.x < HP_COUNT) {
    const int k = threadIdx.x;
    const float coef = s_coef;
#pragma unroll
    for (int g = 0; g < kClipMaxGroups; ++g) {
      if (g < G.ngroups) {
        const float v = G.hp[g][k];
        ws[CLIP_HP_EFF + g * HP_COUNT + k] = k == HP_GRAD_SCALE ? __fmul_rn(v, coef) : v;
      }
    }
  }
}

}  // namespace

hipError_t multi_tensor_clip(const ClipGroups& g, float* clip_ws, hipStream_t s) {
  if (g.ngroups < 1 || g.ngroups > kClipMaxGroups || clip_ws == nullptr) return hipErrorInvalidValue;
  int prev = 0;
  for (int i = 0; i < g.ngroups; ++i) {
    if (!g.tab[i] || !g.chunks[i] || !g.hp[i] || g.c_end[i] <= prev) return hipErrorInvalidValue;
    prev = g.c_end[i];
  }
  const int nchunks = prev;
  // the size rule of multi_tensor_optim_range (PDE_OPTIM_NT overrides it there and here); stores do not occur
  static const int nt_env = std::getenv("PDE_OPTIM_NT") ? std::atoi(std::getenv("PDE_OPTIM_NT")) : -1;
  const int nt = nt_env >= 0 ? nt_env : (static_cast<long>(nchunks) * kOptChunk >= (8L << 20) ? 1 : 0);
  const dim3 grid(static_cast<unsigned>(optim_segment_blocks(nchunks)));
  if (nt != 0) hipLaunchKernelGGL((k_grad_clip<1>), grid, dim3(kOptThreads), 0, s, g, nchunks, clip_ws);
  else hipLaunchKernelGGL((k_grad_clip<0>), grid, dim3(kOptThreads), 0, s, g, nchunks, clip_ws);
  return hipGetLastError();
}

}  // namespace pde
