// variants.hpp -- the builds of a kernel family as a compile-time list, and the one place a run-time key meets it.
// A family states the geometries its planner may choose and the geometries this build holds (the same list unless QA_FAST_BUILD
// cuts it down) as two aliases; its launchers dispatch over the built list and its existence checks ask contains().
#pragma once

#include <type_traits>

namespace qa {

template <int N>
using int_c = std::integral_constant<int, N>;

// one template argument per build: IntList<1, 2, 4>
template <int... N>
struct IntList { static constexpr int values[sizeof...(N)] = {N...}; };

// two template arguments per build: PairList<Pair<4, 3>, Pair<5, 2>>
template <int A, int B>
struct Pair { static constexpr int a = A, b = B; };
template <class... P>
struct PairList {};

// one type per build: TypeList<double, float> (what a kernel family stores its state as); the run-time key is the type's width in bits
template <class T>
struct type_c { using type = T; };
template <class... T>
struct TypeList {};
template <class T>
constexpr int bits_of = 8 * (int)sizeof(T);

// f(the matching entry as integral constants); whether one matched
template <int... N, class F>
bool dispatch(IntList<N...>, int key, F &&f) { return ((key == N && (f(int_c<N>{}), true)) || ...); }
template <class... P, class F>
bool dispatch(PairList<P...>, int a, int b, F &&f) { return ((a == P::a && b == P::b && (f(int_c<P::a>{}, int_c<P::b>{}), true)) || ...); }
template <class... T, class F>
bool dispatch(TypeList<T...>, int bits, F &&f) { return ((bits == bits_of<T> && (f(type_c<T>{}), true)) || ...); }

template <int... N>
constexpr bool contains(IntList<N...>, int key) { return ((key == N) || ...); }
template <class... T>
constexpr bool contains(TypeList<T...>, int bits) { return ((bits == bits_of<T>) || ...); }
template <class... P>
constexpr bool contains(PairList<P...>, int a, int b) { return ((a == P::a && b == P::b) || ...); }

// the largest g(a, b) over the list's entries (a table's extent against a documented range)
template <class... P, class G>
constexpr int max_over(PairList<P...>, G g) {
    int m = 0;
    ((m = g(P::a, P::b) > m ? g(P::a, P::b) : m), ...);
    return m;
}

}  // namespace qa
