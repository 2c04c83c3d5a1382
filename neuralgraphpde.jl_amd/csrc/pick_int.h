// pick_int.h -- one run-time integer to one template argument (host only, plain C++17).
#pragma once

#include <type_traits>

namespace ngpde {

// f(std::integral_constant<int, V>()) for the V of the list that equals v; the last of the list where none does.  A launcher nests
// one call per template argument and names its kernel inside the innermost lambda; a combination that must not be instantiated is
// kept out there with `if constexpr`.
template <int V, int... Vs, class F>
inline void pick_int(int v, F &&f) {
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V>());
  else if (v == V) f(std::integral_constant<int, V>());
  else pick_int<Vs...>(v, f);
}

}  // namespace ngpde
