// dispatch.hpp -- a runtime value turned into a template argument, for launching the kernel instance that matches it.
#pragma once
#include <type_traits>

namespace mk {

// calls f(std::integral_constant<int, V>{}) for the V of Vs... that equals v; false when none does.  The accepted
// values are spelled at the call site, so the set of kernels a launcher instantiates is readable where it launches.
template <int... Vs, typename F>
bool dispatch(int v, F &&f) {
    return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

}  // namespace mk
