// Device primitives of the LDS-DMA kernels (gfx950): the DMA wave-instruction, the
// counted waits and the LDS barrier.  Each kernel keeps its own wave-dependent wait
// tables (wait_own, wait_split, wait_own_k): they encode that kernel's DMA schedule.
#pragma once
#include "rdn_common.h"

template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// LDS-only barrier: this wave's LDS accesses retired, then s_barrier -- NOT
// __syncthreads(), whose vmcnt(0) would also wait for every DMA, load and store in flight
__device__ __forceinline__ void bar_lds() {
  wait_lgkm0();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// One LDS-DMA wave-instruction: 16 B per lane from `src` to LDS byte dst + lane*16
// (dst wave-uniform, in M0).  Inline asm and not the builtin, because the compiler
// must not count it on vmcnt: with the builtin it sees an LDS write pending on the VM
// counter and waits vmcnt(0) before every ds_read of the array, which drains the DMAs
// in flight.  The kernels' explicit counted waits (wait_vm and their wait tables)
// before the publishing barrier are the only ordering.
__device__ __forceinline__ void glds16(const void* src, unsigned dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(src), "s"(__builtin_amdgcn_readfirstlane(dst))
               : "memory");
}
// LDS byte address of a pointer into a __shared__ array
__device__ __forceinline__ unsigned lds_addr(const unsigned char* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)p;
}
