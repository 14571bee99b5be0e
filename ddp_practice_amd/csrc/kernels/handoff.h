// Write-through hand-off of partial results between the workgroups of one launch
// (conv_igemm.hip / conv_wgrad.hip statistics and split-K trees, bn_nhwc.hip ticket trees,
// head.hip CE loss).
//
// Hand-off without fences (MI355X_MICROARCH.md "valid forms", row 1): partial rows are
// written with agent-scope relaxed atomic stores (sc1: write-through past the XCD's L2),
// every wave drains its stores, one relaxed ticket per workgroup; the last arriver reads
// the rows with agent-scope atomic loads.  No release fence: an agent release writes back
// the whole L2 of the XCD (a conv's output tile is dirty in it) once per workgroup.
#pragma once
#include <hip/hip_runtime.h>

namespace dpa {

__device__ __forceinline__ void st_wt(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_wt(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Last-arriver election over `n` workgroups (every thread of the workgroup calls it; true in
// the whole workgroup that arrives last).  wt: the rows were stored write-through (st_wt);
// wt = false is the fenced form (bn_nhwc.set_handoff(0)): an agent-scope release before the
// ticket, an acquire in the last arriver.  The ticket is re-armed by its last arriver (graph
// replays need no reset).
__device__ __forceinline__ bool last_arriver(unsigned* ticket, unsigned n, int* s_flag, bool wt = true) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's partial-row stores are done
  __syncthreads();
  if (threadIdx.x == 0) {
    if (!wt) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = t == n - 1;
    *s_flag = last;
    if (last) {
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
      if (!wt) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
  }
  __syncthreads();
  return *s_flag != 0;
}

}  // namespace dpa
