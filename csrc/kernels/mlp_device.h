// Device helpers shared by the MLP kernels (mlp_fused.hip, mlp_eval.hip): range-checked 16-byte buffer loads, the
// 16x16x32 bf16 MFMA, the LDS-only workgroup barrier and 16-lane row reductions.
#pragma once
#include "common.cuh"

namespace pde {

namespace {

constexpr int OOB = static_cast<int>(0x80000000u);  // a buffer offset past every range: the load returns zeros

using rsrc_t = __amdgpu_buffer_rsrc_t;

__device__ __forceinline__ rsrc_t mkbuf(const void* p, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, static_cast<int>(bytes), 0x00020000);
}
template <int AUX>
__device__ __forceinline__ u16x8 bld16(rsrc_t r, int off) {
  return __builtin_bit_cast(u16x8, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, AUX));
}

__device__ __forceinline__ f32x4 mfma16(const u16x8& a, const u16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                 0, 0);
}

// LDS-only workgroup barrier: LDS accesses complete, then s_barrier -- global loads and stores stay in flight
__device__ __forceinline__ void lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// DPP row (16-lane) reductions: after the four steps every lane holds the op over its row.  Whole wave active.
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <class Op>
__device__ __forceinline__ float row16(float v, Op op) {
  v = op(v, dppf<0xB1>(v));   // quad_perm xor 1
  v = op(v, dppf<0x4E>(v));   // quad_perm xor 2
  v = op(v, dppf<0x141>(v));  // row_half_mirror
  v = op(v, dppf<0x140>(v));  // row_mirror
  return v;
}

}  // namespace

}  // namespace pde
