// The target side shared by the loss kernels (loss.hip, crps_loss.hip): the statistics that normalise a target arriving in physical
// units, t' = (t - mean[var][lev]) / std[var][lev] (reference era5_data/utils_data.py:315-321 `normData`: a subtract, then a true
// division), indexed by LOGICAL level whatever order the target's level axis is stored in.
#pragma once

namespace {

struct TargetStats {                  // null = the target is already normalised
  const float* mean_u; const float* std_u;      // [Vu][L], logical level order
  const float* mean_s; const float* std_s;      // [Vs]
};

bool make_stats(TargetStats& st, const float* mu, const float* su, const float* ms, const float* ss) {
  st = TargetStats{mu, su, ms, ss};
  const int n = (mu != nullptr) + (su != nullptr) + (ms != nullptr) + (ss != nullptr);
  return n == 0 || n == 4;            // all four or none
}

}  // namespace
