// dt_aux_wave.h — blocks the auxiliary kernels' waves start with, each once. A kernel uses a helper only where its
// instruction stream stays the one it had with the block written out (tools/asm_diff.py on the build's .s), judged
// kernel by kernel (DESIGN.md §4 has the table); elsewhere the block stays written out. The __shared__ array stays
// declared in the kernel.
#pragma once
#include "dt_device.h"

// zero the wave's WC_N counters in LDS, barrier, and the Counters over them
__device__ __forceinline__ Counters aux_counters(unsigned int* wc_lds, int lane)
{
  if (lane < WC_N) wc_lds[lane] = 0;
  __syncthreads();
  Counters cnt;
  cnt.wc = wc_lds;
  cnt.box = 0; cnt.prim = 0; cnt.wnodes = 0;
  return cnt;
}

// the launch's scene, parameters and RNG keys, as the trace kernel sets them (pixel and sample: the caller's)
__device__ __forceinline__ Ctx aux_ctx(const DScene& S, const DParams& P)
{
  Ctx c;
  c.S = &S;
  c.P = &P;
  c.rng.k0 = P.seed;
  c.rng.k1 = (uint32_t)P.frame;
  return c;
}
