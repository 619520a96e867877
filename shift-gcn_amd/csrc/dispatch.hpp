// Runtime launch parameters -> template arguments. A launcher is one call:
//
//   const Form form{f.nt, f.lpt};   // or a chooser's tile: with_form<kDw3Tiles>(f.tile, ...)
//   const bool ok = with_form<kJaForms>(form, [&](auto NT, auto LPT, auto RELU, auto RES) {
//     some_kernel<NT, LPT, RELU, RES><<<grid, int(NT), 0, st>>>(...);
//   }, relu != 0, OneOf<0, 1, 2>{res});
//
// The lambda's parameters are std::integral_constants (usable as template arguments). Only
// the listed forms x the flag values are instantiated; a value outside them launches
// nothing and returns false (the entry point then returns SGCN_EINVAL).
#pragma once
#include <tuple>
#include <type_traits>
#include <utility>

namespace sgcn {

// a runtime int that takes one of the values Vs
template <int... Vs>
struct OneOf {
  int v;
};
// a value the caller already fixes at compile time: Const<true>, Const<3>
template <auto V>
using Const = std::integral_constant<decltype(V), V>;

// with_consts(f, a...): each a is a bool, a OneOf or a Const; calls f(constant of a...)
template <class... C>
struct Consts {};   // the constants chosen so far
template <class F, class... C>
bool bind_consts(F& f, Consts<C...>) {
  f(C{}...);
  return true;
}
template <class F, class... C, class T, T V, class... R>
bool bind_consts(F& f, Consts<C...>, std::integral_constant<T, V>, R... r);
template <class F, class... C, int... Vs, class... R>
bool bind_consts(F& f, Consts<C...>, OneOf<Vs...> a, R... r);
template <class F, class... C, class... R>
bool bind_consts(F& f, Consts<C...>, bool a, R... r) {
  return a ? bind_consts(f, Consts<C..., std::true_type>{}, r...)
           : bind_consts(f, Consts<C..., std::false_type>{}, r...);
}
template <class F, class... C, class T, T V, class... R>
bool bind_consts(F& f, Consts<C...>, std::integral_constant<T, V>, R... r) {
  return bind_consts(f, Consts<C..., std::integral_constant<T, V>>{}, r...);
}
template <class F, class... C, int... Vs, class... R>
bool bind_consts(F& f, Consts<C...>, OneOf<Vs...> a, R... r) {
  return ((a.v == Vs && bind_consts(f, Consts<C..., Const<Vs>>{}, r...)) || ...);
}
template <class F, class... A>
bool with_consts(F&& f, A... a) {
  return bind_consts(f, Consts<>{}, a...);
}

// with_form<List>(form, f, a...): f(constants of the fields of form, constants of a...) for
// the entry of List that equals form. List is a constexpr array of a struct whose fields()
// returns its members as a tuple (launch_forms.hpp Form, pw_forms.hpp tiles)
template <const auto& List, size_t I, size_t... J>
auto form_consts(std::index_sequence<J...>) {
  return Consts<Const<std::get<J>(List[I].fields())>...>{};
}
template <const auto& List, size_t I = 0, class F, class... A>
bool with_form(const std::remove_extent_t<std::remove_reference_t<decltype(List)>>& form, F&& f,
               A... a) {
  if constexpr (I == std::extent_v<std::remove_reference_t<decltype(List)>>) {
    return false;
  } else {
    constexpr size_t n = std::tuple_size_v<decltype(List[I].fields())>;
    if (List[I].fields() == form.fields())
      return bind_consts(f, form_consts<List, I>(std::make_index_sequence<n>{}), a...);
    return with_form<List, I + 1>(form, f, a...);
  }
}

}  // namespace sgcn
