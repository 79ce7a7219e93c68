// rbl_schedule.hpp -- the motor schedule of a jointed ensemble run (include/rbl.h section 5, rbl_ensemble_run_jointed): a cycle of
// n_phases phases, phase k lasting phase_steps[k] steps, as the prefix sums cum[0] = 0 < cum[1] < ... < cum[n_phases] = the cycle's
// length.  The map from a position in the cycle to its phase is written here once: the run's kernels evaluate it per replica on
// the device, rbl_run_schedule_phase hands the host's copy of the same statements to the tests.
#pragma once

// the phase k whose half-open range [cum[k], cum[k + 1]) holds p; 0 <= p < cum[n_phases], n_phases >= 1
__host__ __device__ inline int rbl_schedule_phase(const int *cum, int n_phases, int p)
{
  int k = 0;
  while (k + 1 < n_phases && p >= cum[k + 1]) ++k;
  return k;
}

// the position after one committed step
__host__ __device__ inline int rbl_schedule_next(const int *cum, int n_phases, int p)
{
  return p + 1 == cum[n_phases] ? 0 : p + 1;
}
