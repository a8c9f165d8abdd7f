// dispatch.hpp -- run-time values to compile-time ones, for the kernel launch layer (host code only).
//
// A kernel family states ONCE which instantiations ("builds") exist -- a constexpr predicate -- and has one visitor that nests the
// helpers below and hands a generic lambda the kernel of every build the run-time values select.  Launching visits one build;
// configuring (the dynamic-LDS attribute) visits them all by passing EVERY for each value.  Both walk the same lists through the
// same predicate, so no build can be launchable without being configured, or the reverse.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace ti {

constexpr int EVERY = -1;       // in place of a run-time value: visit every listed value

// f(std::integral_constant<int, V>{}) for the V of the list that equals v (every V, in list order: v == EVERY); false: v is not in the list
template <class F>
bool dispatch_int(int, F&&) { return false; }
template <int V, int... Vs, class F>
bool dispatch_int(int v, F&& f)
{
    const bool hit = v == V || v == EVERY;
    if (hit) f(std::integral_constant<int, V>{});
    return dispatch_int<Vs...>(v, f) || hit;
}

// f(std::true_type{}) / f(std::false_type{}) for b = 1 / 0 (a bool converts), both for EVERY
template <class F>
void dispatch_bool(int b, F&& f)
{
    if (b != 0) f(std::true_type{});
    if (b <= 0) f(std::false_type{});
}

// the dynamic-LDS attribute of one kernel: what a family's visitor is handed to configure a build
template <typename K>
hipError_t set_lds(K kernel, size_t bytes)
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace ti
