// Forward-only evaluation of the elastic-DDP MLP (pytorch_elastic/mnist_ddp_elastic.py:117-130, the per-epoch test
// pass over the Linear + ReLU stack of :133-159) as ONE ordinary launch on gfx950: every layer, log-softmax, argmax,
// the hit count and the summed NLL.
//
// Work split.  A workgroup of 256 threads (4 waves) owns ER = 32 consecutive batch rows -- the two 16-row halves of
// one MFMA column block -- and carries them through all layers; the grid is ceil(B / 32).  Workgroups never talk to
// each other except through one arrival ticket at the very end (the totals), and nothing waits on it: a workgroup
// that is not resident simply runs later.  No grid barrier, no spin, no persistent grid, no hand-off through memory.
//
// Activations stay in LDS: two [32][1024 + 8] bf16 buffers used ping-pong.  Layer l reads its A fragments from one
// (one 16-byte LDS read per lane: row lane & 15, k = 32 ks + 8 (lane >> 4) .. + 7) and writes relu(acc + bias),
// rounded with f2bf, into the other; one workgroup barrier per layer.  Row pitch: 1032 bf16 = 2064 bytes =
// 8 x 256 + 16, so row r starts 16 r bytes (mod 256) into the 64 banks x 4 bytes: the 16 rows that one quarter-wave
// reads at a common k fall on 16 distinct 16-byte bank groups, i.e. every bank exactly once -- no conflict; 16-byte
// alignment holds because 2064 = 16 x 129.  Layer 0's A operand is the fp32 input, rounded to bf16 while it is staged;
// rows >= B and the columns from K up to the next multiple of 32 are zero (every layer's epilogue zero-fills the
// same way: its padded N-tiles see zero weights and a zero bias), so a K tail multiplies zeros, never stale LDS.
//
// Weights go straight from memory into MFMA B fragments: with v_mfma_f32_16x16x32_bf16 a lane's B fragment is 8
// consecutive k of one output column = 16 contiguous bytes of the row-major [out][in] bf16 copy, and each fragment
// is used by exactly one wave, so LDS would only add a round trip.  Loads go through a buffer descriptor sized to
// the tensor (an out-of-range fragment is requested at an offset past every range and reads as zeros) into a
// register ring of ERING k-steps: a slot is re-requested for the wave's next chunk right behind the two MFMAs (one
// per 16-row half) that consumed it, across tile boundaries, and the first chunk of the NEXT layer is requested
// before the layer's barrier.
//
// N-tiles of 16 columns are dealt round-robin to the four waves and a wave runs the whole K of its tile alone:
// no K split, no cross-wave reduction, a fixed accumulation order.  The last layer (out <= 16: one N-tile) splits K
// over the four waves instead (k-step ks on wave ks % 4), sums the quarters through LDS in wave order, and wave 0
// takes the per-row log-softmax, the argmax (lowest index on a tie) and -logp[y] with 16-lane row operations.
//
// Totals: CnnEvalStats' layout and protocol (cnn_fused.hip k_cnn_eval) -- a per-workgroup NLL partial, an integer
// atomic for the hits, one ticket; the last workgroup to draw it sums the partials in workgroup order, adds them to
// the running totals and resets the ticket.  Equal calls give bitwise-equal totals; a second call adds.
#include "common.cuh"
#include "mlp_device.h"
#include "mlp_eval.h"

namespace pde {

namespace {

constexpr int ET = 256;            // 4 waves
constexpr int ER = 32;             // batch rows per workgroup
constexpr int EKMAX = 1024;        // widest layer input
constexpr int EPITCH = EKMAX + 8;  // bf16 per activation row (see the bank arithmetic above)
constexpr int ERING = 8;           // k-steps (of 32) in flight per wave: 8 x 64 lanes x 16 bytes = 8 KB
constexpr int EAHEAD = 4;          // k-steps the LDS reads of the A fragments run ahead of their MFMAs

struct EvalSmem {
  uint16_t act[2][ER * EPITCH];  // ping-pong activations, 2 x 66,048 bytes
  f32x4 red[3][2][64];           // last layer: waves 1..3's K-quarter partials
};
static_assert(sizeof(EvalSmem) <= 160 * 1024, "LDS budget");
static_assert((EPITCH * 2) % 256 == 16 && EPITCH >= EKMAX, "row pitch: 16 rows on 16 distinct 16-byte bank groups");
static_assert(EAHEAD >= 1 && EAHEAD < ERING, "the A ring is ERING slots deep");
static_assert(4 * ERING * 32 >= EKMAX, "the last layer holds its whole K quarter in the ring");

// The running totals of CnnEvalStats (models/cnn_fused.py): four 8-byte words.
struct EvalTotals {
  double loss_sum;
  unsigned long long correct, count, ticket;
};
static_assert(sizeof(EvalTotals) == 32, "CnnEvalStats holds int64[4]");

// A hidden layer as one wave streams it: N-tile t, chunk c of ERING k-steps
struct Tiles {
  rsrc_t rw;
  int N, K, nks, nc, ntp;  // k-steps, chunks per tile, N-tiles padded to an even count (32 zero-filled columns)
};
__device__ __forceinline__ Tiles mk_tiles(const MlpEvalLayer& L) {
  Tiles T;
  T.rw = mkbuf(L.w, static_cast<long>(L.out) * L.in * 2);
  T.N = L.out;
  T.K = L.in;
  T.nks = (L.in + 31) >> 5;
  T.nc = (T.nks + ERING - 1) / ERING;
  T.ntp = ((L.out + 31) >> 5) * 2;
  return T;
}
// B fragment of tile t, k-step ks: W[16 t + (lane & 15)][32 ks + 8 (lane >> 4) .. + 7]; zeros outside the tensor
__device__ __forceinline__ u16x8 ldb(const Tiles& T, int t, int ks, int lane) {
  const int n = t * 16 + (lane & 15), k = ks * 32 + 8 * (lane >> 4);
  return bld16<0>(T.rw, n < T.N && k < T.K ? (n * T.K + k) * 2 : OOB);
}
__device__ __forceinline__ void prime_hidden(const MlpEvalLayer& L, u16x8 (&ring)[ERING], int w, int lane) {
  const Tiles T = mk_tiles(L);
#pragma unroll
  for (int j = 0; j < ERING; ++j) ring[j] = ldb(T, w, j, lane);
}
// The last layer's K quarter of wave w: k-steps w, w + 4, ..
__device__ __forceinline__ void prime_last(const MlpEvalLayer& L, u16x8 (&ring)[ERING], int w, int lane) {
  const Tiles T = mk_tiles(L);
#pragma unroll
  for (int u = 0; u < ERING; ++u) ring[u] = ldb(T, 0, w + 4 * u, lane);
}

__device__ __forceinline__ float tile_bias(const MlpEvalLayer& L, int t, int lane) {
  const int n = t * 16 + (lane & 15);
  return n < L.out ? L.b[n] : 0.f;
}

// One hidden layer for this wave: nxt[:, tiles w, w + 4, ..] = bf16(relu(cur . W^T + b)).  ring holds the first
// chunk of tile w on entry.  A k-step past the layer's last one re-reads the last A fragment against a zero B.
__device__ __forceinline__ void hidden_layer(const MlpEvalLayer& L, const uint16_t* cur, uint16_t* nxt,
                                             u16x8 (&ring)[ERING], int w, int lane) {
  const Tiles T = mk_tiles(L);
  const int chunks = T.ntp > w ? ((T.ntp - w + 3) >> 2) * T.nc : 0;
  const uint16_t* a0p = cur + (lane & 15) * EPITCH + 8 * (lane >> 4);
  const uint16_t* a1p = a0p + 16 * EPITCH;
  int ut = w, uc = 0, lt = w, lc = 1;  // the tile / chunk in use, and the next one to request
  if (lc == T.nc) {
    lc = 0;
    lt += 4;
  }
  f32x4 c0{0.f, 0.f, 0.f, 0.f}, c1 = c0;
  float bias = tile_bias(L, ut, lane);
  // A fragments run EAHEAD k-steps ahead of their MFMAs in a register ring of their own, across chunk and tile
  // boundaries (every tile re-reads the same rows from k = 0), so an LDS read has 2 x EAHEAD MFMAs to complete under
  const auto lda = [&](const uint16_t* p, int ks) {
    return *reinterpret_cast<const u16x8*>(p + (ks < T.nks ? ks : T.nks - 1) * 32);
  };
  u16x8 a0[ERING], a1[ERING];
#pragma unroll
  for (int j = 0; j < EAHEAD; ++j) {
    a0[j] = lda(a0p, j);
    a1[j] = lda(a1p, j);
  }
  for (int q = 0; q < chunks; ++q) {
    const int kn = (uc + 1 == T.nc ? 0 : uc + 1) * ERING;  // the next chunk's first k-step
#pragma unroll
    for (int j = 0; j < ERING; ++j) {
      const int jn = (j + EAHEAD) % ERING;
      const int ksn = j + EAHEAD < ERING ? uc * ERING + j + EAHEAD : kn + jn;
      a0[jn] = lda(a0p, ksn);
      a1[jn] = lda(a1p, ksn);
      c0 = mfma16(a0[j], ring[j], c0);
      c1 = mfma16(a1[j], ring[j], c1);
      ring[j] = ldb(T, lt, lc * ERING + j, lane);
    }
    if (++lc == T.nc) {
      lc = 0;
      lt += 4;
    }
    if (++uc == T.nc) {
      // accumulator layout: c[r] = row 4 (lane >> 4) + r of the half, column lane & 15 of the tile
      uint16_t* o = nxt + 4 * (lane >> 4) * EPITCH + ut * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v0 = c0[r] + bias, v1 = c1[r] + bias;
        o[r * EPITCH] = f2bf(v0 < 0.f ? 0.f : v0);
        o[(16 + r) * EPITCH] = f2bf(v1 < 0.f ? 0.f : v1);
      }
      uc = 0;
      ut += 4;
      c0 = f32x4{0.f, 0.f, 0.f, 0.f};
      c1 = c0;
      bias = tile_bias(L, ut, lane);
    }
  }
}

__global__ __launch_bounds__(ET) void k_mlp_eval(const MlpEvalArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  EvalSmem& S = *reinterpret_cast<EvalSmem*>(smem_raw);
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int m0 = blockIdx.x * ER, B = a.B, nl = a.nl;
  u16x8 ring[ERING];

  // ---- layer 0's first weight chunk is requested first; then the input rows: fp32 -> bf16 into act[0], 8 threads
  // per row, 32 bytes per thread and pass, zeros for rows >= B and for k in [K, 32 ceil(K / 32))
  prime_hidden(a.L[0], ring, w, lane);
  {
    const int K = a.L[0].in, groups = ((K + 31) >> 5) * 4, row = t >> 3, r = m0 + row;
    const float* xr = a.x + static_cast<long>(r < B ? r : 0) * K;
#pragma unroll 4
    for (int g = t & 7; g < groups; g += 8) {
      const int k = 8 * g;
      u16x8 o{0, 0, 0, 0, 0, 0, 0, 0};
      if (r < B && k < K) {
        const f32x4* q = reinterpret_cast<const f32x4*>(xr + k);
        const f32x4 x0 = q[0], x1 = q[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o[j] = f2bf(x0[j]);
          o[4 + j] = f2bf(x1[j]);
        }
      }
      *reinterpret_cast<u16x8*>(&S.act[0][row * EPITCH + k]) = o;
    }
  }
  lds_sync();

  // ---- hidden layers, ping-pong; the next layer's first chunk is requested ahead of the barrier
  int cur = 0;
  for (int l = 0; l < nl - 1; ++l) {
    hidden_layer(a.L[l], S.act[cur], S.act[cur ^ 1], ring, w, lane);
    if (l + 1 < nl - 1)
      prime_hidden(a.L[l + 1], ring, w, lane);
    else
      prime_last(a.L[l + 1], ring, w, lane);
    lds_sync();
    cur ^= 1;
  }

  // ---- last layer: K quarters on the four waves, summed through LDS in wave order
  const MlpEvalLayer& F = a.L[nl - 1];
  const int N = F.out, col = lane & 15;
  const bool valid = col < N;
  const float fbias = valid ? F.b[col] : 0.f;
  int y[2][4];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + 16 * s + 4 * (lane >> 4) + r;
      y[s][r] = (a.tgt != nullptr && row < B) ? static_cast<int>(a.tgt[row]) : -1;
    }
  f32x4 c0{0.f, 0.f, 0.f, 0.f}, c1 = c0;
  {
    const int nks = (F.in + 31) >> 5;
    const uint16_t* a0p = S.act[cur] + (lane & 15) * EPITCH + 8 * (lane >> 4);
    const uint16_t* a1p = a0p + 16 * EPITCH;
#pragma unroll
    for (int u = 0; u < ERING; ++u) {
      const int ks = w + 4 * u, ka = (ks < nks ? ks : nks - 1) * 32;
      c0 = mfma16(*reinterpret_cast<const u16x8*>(a0p + ka), ring[u], c0);
      c1 = mfma16(*reinterpret_cast<const u16x8*>(a1p + ka), ring[u], c1);
    }
  }
  if (w > 0) {
    S.red[w - 1][0][lane] = c0;
    S.red[w - 1][1][lane] = c1;
  }
  lds_sync();
  if (w != 0) return;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    c0 += S.red[q][0][lane];
    c1 += S.red[q][1][lane];
  }

  // ---- head (wave 0): a row's 16 columns sit in the 16 lanes of a DPP row
  float nll = 0.f, hits = 0.f;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + 16 * s + 4 * (lane >> 4) + r;
      const bool ok = row < B;
      const float logit = (s ? c1[r] : c0[r]) + fbias;
      const float m = row16(valid ? logit : -INFINITY, [](float p, float q) { return fmaxf(p, q); });
      const float d = logit - m;
      const float sum = row16(valid ? expf(d) : 0.f, [](float p, float q) { return p + q; });
      const float lp = d - logf(sum);
      const float am = row16((valid && logit == m) ? static_cast<float>(col) : 16.f,
                             [](float p, float q) { return fminf(p, q); });
      const int pr = am < 16.f ? static_cast<int>(am) : 0;  // (no lane equals the maximum only for NaN logits)
      const float ly = row16((valid && col == y[s][r]) ? -lp : 0.f, [](float p, float q) { return p + q; });
      if (ok && valid) {
        const long e = static_cast<long>(row) * N + col;
        if (a.logits != nullptr) a.logits[e] = logit;
        if (a.logp != nullptr) a.logp[e] = lp;
      }
      if (ok && col == 0) {
        if (a.pred != nullptr) a.pred[row] = pr;
        nll += ly;
        hits += pr == y[s][r] ? 1.f : 0.f;
      }
    }
  if (a.stats == nullptr) return;

  // ---- totals.  The workgroup publishes its rows' NLL sum and adds its hits (integer atomic); the last one to
  // draw a ticket sums the partials in workgroup order -- the same value whatever order the workgroups finished
  // in -- adds it to the running total and resets the ticket for the next launch or replay.
  EvalTotals* stats = static_cast<EvalTotals*>(a.stats);
  const float l = wave_sum(nll);
  const int h = static_cast<int>(wave_sum(hits));  // at most 32: exact
  unsigned long long old = 0;
  if (lane == 0) {
    __hip_atomic_store(&a.loss_part[blockIdx.x], l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
      sum += __hip_atomic_load(&a.loss_part[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sum = wave_sum(sum);
    if (lane == 0) {
      stats->loss_sum += static_cast<double>(sum);
      stats->count += static_cast<unsigned long long>(B);
      __hip_atomic_store(&stats->ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace

int mlp_eval_rows_per_workgroup() { return ER; }

hipError_t mlp_eval(const MlpEvalArgs& a, hipStream_t s) {
  if (a.nl < 2 || a.nl > kMlpMaxLayers || a.B < 1 || a.x == nullptr) return hipErrorInvalidValue;
  for (int l = 0; l < a.nl; ++l) {
    const MlpEvalLayer& L = a.L[l];
    const bool last = l == a.nl - 1;
    if (L.w == nullptr || L.b == nullptr || L.in < 8 || L.in % 8 || L.in > EKMAX) return hipErrorInvalidValue;
    if (last ? (L.out < 1 || L.out > 16) : (L.out < 8 || L.out % 8 || L.out > EKMAX)) return hipErrorInvalidValue;
    if (l > 0 && L.in != a.L[l - 1].out) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(L.w) & 15) return hipErrorInvalidValue;  // 16-byte fragment loads
  }
  if ((reinterpret_cast<uintptr_t>(a.x) & 15) || (reinterpret_cast<uintptr_t>(a.stats) & 7))
    return hipErrorInvalidValue;
  if (a.stats != nullptr && (a.tgt == nullptr || a.loss_part == nullptr)) return hipErrorInvalidValue;
  const size_t sm = sizeof(EvalSmem);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mlp_eval), hipFuncAttributeMaxDynamicSharedMemorySize,
                              static_cast<int>(sm));
    attr = true;
  }
  hipLaunchKernelGGL(k_mlp_eval, dim3(ceil_div(a.B, ER)), dim3(ET), sm, s, a);
  return hipGetLastError();
}

}  // namespace pde
