// sgk_shapes.h -- the shapes the kernels are instantiated for, each list once, with the dispatch from run-time values to template
// arguments and the predicate the C-ABI layer refuses by: the conv bodies' board shapes and channel counts (acting kernels and
// learner alike), the MLP bodies' hidden widths (acting / learning) and board sizes. Host code only; every level of
// sgk_level_table.h is checked against the lists at compile time.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "sgk_level_table.h"

namespace sgk {

// A list of ints: sizes_listed says whether v is in it; sizes_dispatch calls f(std::integral_constant<int, v>) for the listed v and
// returns what f returns, hipErrorInvalidValue for any other v.
template <int... V>
struct Sizes {};
template <int... V>
constexpr bool sizes_listed(Sizes<V...>, int v) {
  return ((V == v) || ...);
}
template <int... V, class F>
hipError_t sizes_dispatch(Sizes<V...>, int v, F &&f) {
  hipError_t err = hipErrorInvalidValue;
  (void)((V == v && (err = f(std::integral_constant<int, V>{}), true)) || ...);
  return err;
}

typedef Sizes<5, 4, 8> CqChannels;            // conv bodies: policy_cnn.py's default, and the two powers of two around it
typedef Sizes<64, 100, 128> MlpActWidths;     // MLP acting kernels: the reference default (100) and the two common powers of two
typedef Sizes<64, 100> MlpLearnWidths;        // MLP learners (DQN, PPO)

// The board shapes the conv kernels are built for. cq_dispatch calls f(board, channels) with the compile-time values of the listed
// board that is height x width and of n_channels (f's `board` has ::H and ::W, `channels` ::value) and returns what f returns;
// hipErrorInvalidValue where nothing is listed. The rollout, whose board follows from its level, takes the channel half alone.
template <int H_, int W_>
struct CqBoard {
  static constexpr int H = H_, W = W_;
};
template <class... B>
struct CqBoards {};
typedef CqBoards<CqBoard<5, 5>, CqBoard<6, 5>, CqBoard<6, 6>, CqBoard<6, 8>, CqBoard<7, 7>, CqBoard<7, 8>, CqBoard<7, 9>> CqOneBoardShapes;
typedef CqBoards<CqBoard<5, 5>> CqTwoBoardShapes;  // BoatRace, the level TransitionBoatRace wraps; another level is one more entry

template <class F>
hipError_t cq_dispatch_channels(int n_channels, F &&f) {
  return sizes_dispatch(CqChannels{}, n_channels, f);
}
template <class... B, class F>
hipError_t cq_dispatch(CqBoards<B...>, int height, int width, int n_channels, F &&f) {
  hipError_t err = hipErrorInvalidValue;
  (void)((B::H == height && B::W == width && (err = cq_dispatch_channels(n_channels, [&](auto channels) { return f(B{}, channels); }), true)) || ...);
  return err;
}
template <class... B>
constexpr bool cq_board_listed(CqBoards<B...>, int height, int width) {
  return ((B::H == height && B::W == width) || ...);
}

// The board sizes (cells) the MLP kernels are instantiated for -- policy forward, DQN and PPO learners. SGK_DISPATCH_CELLS binds K0; a
// size without a kernel returns hipErrorInvalidValue from the calling function.
#define SGK_MLP_CELLS(X, ...) X(25, __VA_ARGS__) X(30, __VA_ARGS__) X(36, __VA_ARGS__) X(48, __VA_ARGS__) X(49, __VA_ARGS__) X(56, __VA_ARGS__) X(63, __VA_ARGS__)
#define SGK_MLP_CELLS_CASE(N, ...) case N:
constexpr bool mlp_cells_listed(int n_cells) {
  switch (n_cells) {
    SGK_MLP_CELLS(SGK_MLP_CELLS_CASE, )
    return true;
  default: return false;
  }
}
#undef SGK_MLP_CELLS_CASE
#define SGK_DISPATCH_CELLS_ARM(N, ...) \
  case N: {                            \
    constexpr int K0 = N;              \
    __VA_ARGS__;                       \
  } break;
#define SGK_DISPATCH_CELLS(NCELLS, ...)                        \
  do {                                                         \
    switch (NCELLS) {                                          \
      SGK_MLP_CELLS(SGK_DISPATCH_CELLS_ARM, __VA_ARGS__)       \
    default: return hipErrorInvalidValue;                      \
    }                                                          \
  } while (0)

// every level has an MLP kernel of its size and a one-board conv kernel of its shape: a new level that does not fails here
#define SGK_LEVEL_COVERED(ID, P, ...)                                                                                  \
  static_assert(mlp_cells_listed(Geom<ID>::NC), "SGK_MLP_CELLS lacks this level's board size");                        \
  static_assert(cq_board_listed(CqOneBoardShapes{}, Geom<ID>::H, Geom<ID>::W), "CqOneBoardShapes lacks this level's board shape");
SGK_LEVEL_LIST(SGK_LEVEL_COVERED, )
#undef SGK_LEVEL_COVERED

}  // namespace sgk
