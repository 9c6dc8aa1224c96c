// scn_dispatch.h -- run-time launch parameters turned into template arguments, once for every launcher.  Host only.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "scn_wire.h"

// f(integral_constant<int, KIND>, bool_constant<DC>) for the wire format `kind`; DC is false for float samples whatever `dc`
// says (no DC removal there, messageQueue.h:229-236).  Unknown kind: hipErrorInvalidValue.
template <class F>
hipError_t scn_with_kind(int kind, bool dc, F &&f) {
  auto with_dc = [&](auto k) { return dc ? f(k, std::true_type{}) : f(k, std::false_type{}); };
  switch (kind) {
    case SCN_K_FLOAT_COMPLEX: return f(std::integral_constant<int, SCN_K_FLOAT_COMPLEX>{}, std::false_type{});
    case SCN_K_SHORT_COMPLEX: return with_dc(std::integral_constant<int, SCN_K_SHORT_COMPLEX>{});
    case SCN_K_SHORT: return with_dc(std::integral_constant<int, SCN_K_SHORT>{});
    case SCN_K_BYTE_COMPLEX: return with_dc(std::integral_constant<int, SCN_K_BYTE_COMPLEX>{});
    default: return hipErrorInvalidValue;
  }
}
// the same for the families that take DC removal at run time: f(integral_constant<int, KIND>), one instantiation per format
template <class F>
hipError_t scn_with_kind(int kind, F &&f) {
  return scn_with_kind(kind, false, [&](auto k, auto) { return f(k); });
}

// Output mode of a launch, f(bool_constant<HITS>, bool_constant<SPEC>), the three legal ones:
//   hits && spec: spectrum + hits;   !hits: spectrum only;   hits && !spec: hits only (no stores, no per-bin logarithm)
template <class F>
auto scn_with_mode(bool hits, bool spec, F &&f) {
  if (!hits) return f(std::false_type{}, std::true_type{});
  if (spec) return f(std::true_type{}, std::true_type{});
  return f(std::true_type{}, std::false_type{});
}
