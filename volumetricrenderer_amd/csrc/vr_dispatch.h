// vr_dispatch.h -- runtime value -> compile-time tag, for the march launchers (host only).
//
// Every march kernel is a template over compile-time choices (layout, wrap, EARLY, ZO, the
// uniform channel, NF, split K, workgroup width, SHADOW / TABLE) and the host picks the
// instantiation from runtime values.  A launcher states that choice as nested calls of the
// three functions below around one generic lambda that names the kernel once:
//
//     with_bool(early, [&](auto E) { return with_bool(zo, [&](auto Z) {
//         hipLaunchKernelGGL((march_regions<L, W, E, Z>), ...);   // E, Z: std::bool_constant
//         return hipGetLastError(); }); });
//
// A tag converts to its value in a constant expression, so it is a template argument and
// an `if constexpr` condition as it stands; `if constexpr` inside the lambda prunes the
// instantiations a launcher does not build.  Only the listed values are instantiated.
#pragma once
#include <hip/hip_runtime_api.h>   // hipError_t
#include <type_traits>

namespace vr {

// f(std::true_type{}) or f(std::false_type{})
template <class F>
decltype(auto) with_bool(bool b, F&& f)
{
    if (b) return f(std::true_type{});
    return f(std::false_type{});
}

// f(std::integral_constant<int, V>{}) for the first V of Vs equal to v; else `otherwise`
template <int... Vs, class F, class R>
R with_value(int v, F&& f, R otherwise)
{
    (void)((v == Vs ? (otherwise = f(std::integral_constant<int, Vs>{}), true) : false) || ...);
    return otherwise;
}

// A named list of values (the layouts a translation unit instantiates, vr_internal.h)
template <int... Vs>
struct value_list {};
template <class A, class B>
struct list_cat;
template <int... As, int... Bs>
struct list_cat<value_list<As...>, value_list<Bs...>> {
    using type = value_list<As..., Bs...>;
};
template <class A, class B>
using list_cat_t = typename list_cat<A, B>::type;
template <int... Vs>
constexpr bool list_has(value_list<Vs...>, int v)
{
    return ((v == Vs) || ...);
}

// with_value over a named list.  A layout the list does not hold is an error, never
// another kernel.
template <int... Ls, class F>
hipError_t with_layout(value_list<Ls...>, int layout, F&& f)
{
    return with_value<Ls...>(layout, f, hipErrorInvalidValue);
}
template <class LayoutList, class F>
hipError_t with_layout(int layout, F&& f)
{
    return with_layout(LayoutList{}, layout, f);
}

}  // namespace vr
