// Matrix-core and direct-to-LDS primitives shared by the MFMA kernels (device code only; include after aid_common.h).
#pragma once
#include <stdint.h>
#include <type_traits>
#include <utility>

typedef float f32x16 __attribute__((ext_vector_type(16)));      // the accumulator of one 32 x 32 MFMA tile
typedef float f32x4 __attribute__((ext_vector_type(4)));        // the accumulator of one 16 x 16 MFMA tile: lane l holds rows 4 (l / 16) + r, column l % 16

// 16-byte direct-to-LDS load through the compiler builtin: the compiler tracks it and places the waits.
#define AID_GLDS16(gptr, lptr) \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gptr), (__attribute__((address_space(3))) void*)(lptr), 16, 0, 0)

// Direct-to-LDS loads issued through inline asm (used by the kernels that keep several LDS buffers in flight: the row-shared Winograd-domain-input kernels and the 2-D Winograd GEMM family): the compiler's
// waitcnt insertion cannot tell which LDS buffer a global_load_lds writes and would drain vmcnt before the next ds_read of
// ANY buffer; issued this way it does not see them and the kernel places its own s_waitcnt vmcnt(n).  vmcnt completes in
// order, so every wait the compiler emits for its own loads stays correct (it can only over-wait).  M0 is a reserved
// register: nothing else in these kernels keeps a value in it.
#define AID_LDS_ADDR(lptr) ((unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)(lptr))
#define AID_DMA16_RAW(gptr, lds_addr) \
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(gptr), "s"(lds_addr) : "memory")
// the same with a SCALAR 64-bit base and a 32-bit per-lane byte offset (one VGPR per piece instead of a 64-bit pointer and a per-lane stride)
#define AID_DMA16_SBASE(voff, sbase, lds_addr) \
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voff), "s"(sbase), "s"(lds_addr) : "memory")
// s_waitcnt immediates (gfx9 encoding: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt[5:4] << 14)
#define AID_VMCNT(n) ((((n) & 15) | (7 << 4) | (15 << 8) | ((((n) >> 4) & 3) << 14)))
#define AID_LGKMCNT0 (15 | (7 << 4) | (0 << 8) | (3 << 14))

template <typename F, int... I>
__device__ __forceinline__ void aid_static_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void aid_static_for(F&& f) { aid_static_for_impl(f, std::make_integer_sequence<int, N>{}); }
// s_waitcnt vmcnt(n) for a wave-uniform n in [0, NMAX] (the instruction takes an immediate)
template <int NMAX>
__device__ __forceinline__ void aid_wait_vmcnt_le(int n) {
    if constexpr (NMAX == 0) { __builtin_amdgcn_s_waitcnt(AID_VMCNT(0)); }
    else { if (n >= NMAX) __builtin_amdgcn_s_waitcnt(AID_VMCNT(NMAX)); else aid_wait_vmcnt_le<NMAX - 1>(n); }
}
