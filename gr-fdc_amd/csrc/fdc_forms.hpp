// Host: which instantiation of a kernel a launch takes.  A kernel file states the forms of its kernel ONCE, as a walker over the lists of its template
// arguments; "set the LDS attribute of every instantiation" is that walker with kEvery, "launch the one that matches" is the walker with the launch's
// values.  So a form that can be launched has its attribute set by construction, and a request without a form leaves the launcher's error as it was.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace fdc {

// f(std::integral_constant<int, V>{}) for the V that equals v, or for every V (v = kEvery)
constexpr int kEvery = -1;
template <int... Vs, class F>
inline void for_values(int v, F &&f)
{
    ((v == kEvery || v == Vs ? f(std::integral_constant<int, Vs>{}) : void()), ...);
}
inline hipError_t set_block_lds(const void *kernel, int bytes)
{
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

}  // namespace fdc
