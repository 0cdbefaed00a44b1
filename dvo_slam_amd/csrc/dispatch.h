// dispatch.h -- a runtime value as a compile-time one: the launchers pick a kernel instantiation with these (host code).
//   with_bool(stream_nt, [&](auto NT) { k<decltype(NT)::value><<<...>>>(...); });
//   with_value<0, 1, -1>(role, [&](auto ROLE) { ... });      a value that is none of those listed takes the LAST one
// An illegal combination is left out with `if constexpr` inside the callable, so it is never instantiated.
#pragma once
#include <type_traits>

namespace dvo_hip {

template <typename F>
void with_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}

template <int V, int... Rest, typename F>
void with_value(int v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, V>{});
  else if (v == V) f(std::integral_constant<int, V>{});
  else with_value<Rest...>(v, f);
}

}  // namespace dvo_hip
