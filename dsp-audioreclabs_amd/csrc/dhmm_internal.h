// dhmm_internal.h -- what dhmm.hip (isolated words) and dhmm_decode.hip (connected words) share: the
// bounds of a discrete-HMM model set and the register slots of a launch.
#pragma once

namespace dsp {

static constexpr int DHMM_SMAX = 32;   // states a lane keeps in registers at most
static constexpr int DHMM_KMAX = 256;  // symbols of the alphabet at most

// register slots of a launch: the smallest of 8, 16, 32 that holds Smax
static inline int dhmm_slots(int Smax) { return Smax <= 8 ? 8 : (Smax <= 16 ? 16 : 32); }

}  // namespace dsp
