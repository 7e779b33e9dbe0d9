// What the Mask2Former matcher (m2f_match.hip) and criterion (m2f_loss.hip) share on the host side of their entry points: the cap on
// the prediction steps of a call, the shape predicate for S, and the one function that turns a caller's per-step pointer table into
// the table a kernel takes BY VALUE. The table types themselves are the public ones of include/mss_hip.h (MssM2fMaps, MssM2fSteps,
// MssM2fGrads: plain arrays of MSS_M2F_MAX_STEPS device pointers), so a kernel argument and a caller's struct have one layout.
#pragma once
#include "../../include/mss_hip.h"

inline bool m2f_steps_ok(int S) { return S >= 1 && S <= MSS_M2F_MAX_STEPS; }

// dev[0 .. S) = host[0 .. S), none of them NULL; dev[S ..) = NULL whatever the caller left there. S: m2f_steps_ok.
template <typename T>
inline bool m2f_fill(T* (&dev)[MSS_M2F_MAX_STEPS], T* const* host, int S) {
  if (!host) return false;
  for (int s = 0; s < MSS_M2F_MAX_STEPS; ++s) {
    if (s < S && !host[s]) return false;
    dev[s] = s < S ? host[s] : nullptr;
  }
  return true;
}
