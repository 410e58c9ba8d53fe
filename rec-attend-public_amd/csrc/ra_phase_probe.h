// In-kernel phase probe of the persistent conv kernels: wave 0 of every workgroup accumulates the shader-clock time it spends
// between a few points of its tile loop (RA_PHASE_AT(k), k = 0..6) and leaves the sums, with the wall-clock time of the whole
// walk in slot 7, in buf[workgroup][8].  Built only by the stand-alone probes under tools/, each with its file's own flag.
//
// A file that carries probe points defines, under its flag and before it includes this header,
//   RA_PHASE_PROBE_BUF  its `__device__ long long *` buffer symbol (null = the launch is not probed)
//   RA_PHASE_PROBE_WG   the workgroup's index in the grid
// and writes RA_PHASE_DECL once at the top of the kernel, RA_PHASE_AT(k) at the points and RA_PHASE_END at its end.  Without
// the two names all three expand to nothing.
#pragma once

#ifdef RA_PHASE_PROBE_BUF
#define RA_PHASE_DECL long long ph_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ph_t = (long long)__builtin_readcyclecounter(), ph_t0 = (long long)wall_clock64()
#define RA_PHASE_AT(k)                                            \
  do {                                                            \
    __builtin_amdgcn_sched_barrier(0);                            \
    const long long n_ = (long long)__builtin_readcyclecounter(); \
    ph_acc[k] += n_ - ph_t;                                       \
    ph_t = n_;                                                    \
    __builtin_amdgcn_sched_barrier(0);                            \
  } while (0)
#define RA_PHASE_END                                                                                          \
  do {                                                                                                        \
    if (threadIdx.x == 0 && RA_PHASE_PROBE_BUF) {                                                             \
      ph_acc[7] = (long long)wall_clock64() - ph_t0;                                                          \
      for (int k_ = 0; k_ < 8; ++k_) RA_PHASE_PROBE_BUF[(size_t)(RA_PHASE_PROBE_WG) * 8 + k_] = ph_acc[k_]; \
    }                                                                                                         \
  } while (0)
#else
#define RA_PHASE_DECL
#define RA_PHASE_AT(k)
#define RA_PHASE_END
#endif
