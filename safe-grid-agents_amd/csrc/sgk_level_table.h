// sgk_level_table.h -- the levels as compile-time constants: the board geometry the kernels are specialised on and the dispatch from a
// run-time level id to a template argument, both generated from SGK_LEVEL_LIST (include/sgk_levels.h), the one list of levels. Plain
// C++: included by the kernels (through sgk_transition.h) and by the host-only debug library that g++ builds.
#pragma once
#include "../../include/sgk.h"
#include "../../include/sgk_levels.h"

namespace sgk {

// a PITCHED board row: the level's cells padded to whole 16-byte stores
constexpr int pitched_row_bytes(int n_cells) { return (n_cells + 15) / 16 * 16; }

template <int ENV>
struct Geom;
#define SGK_LEVEL_GEOM(ID, P, ...)                                                                                              \
  static_assert(SGK_ENV_##P == ID, "sgk_levels.h and sgk.h number the levels alike");                                           \
  template <>                                                                                                                   \
  struct Geom<ID> {                                                                                                             \
    static constexpr int H = SGK_##P##_H, W = SGK_##P##_W, NC = H * W, PITCH = pitched_row_bytes(NC);                            \
  };                                                                                                                            \
  static_assert(Geom<ID>::H <= SGK_MAX_H && Geom<ID>::W <= SGK_MAX_W && Geom<ID>::NC <= SGK_MAX_CELLS, "board within the rule tables");
SGK_LEVEL_LIST(SGK_LEVEL_GEOM, )
#undef SGK_LEVEL_GEOM

#define SGK_LEVEL_CASE(ID, P, ...) case ID:
constexpr bool level_listed(int env_id) {
  switch (env_id) {
    SGK_LEVEL_LIST(SGK_LEVEL_CASE, )
    return true;
  default: return false;
  }
}
#undef SGK_LEVEL_CASE
// What the dispatch below takes an id outside the list for: Sokoban, as its `default:` arm always did. No caller can pass one -- a
// handle exists only for an id sgk_build_rules knows (sgk_create_ex), and the debug hooks ask level_listed first.
constexpr int dispatched_level(int env_id) { return level_listed(env_id) ? env_id : SGK_SIDE_EFFECTS_SOKOBAN; }

}  // namespace sgk

// Runs the statement(s) after ENVID with E bound to the level as a constant expression; with LAYOUT, L to the board layout as well.
#define SGK_DISPATCH_ENV_ARM(ID, P, ...) \
  case ID: {                             \
    constexpr int E = ID;                \
    __VA_ARGS__;                         \
  } break;
#define SGK_DISPATCH_ENV(ENVID, ...)                                                                \
  do {                                                                                              \
    switch (sgk::dispatched_level(ENVID)) { SGK_LEVEL_LIST(SGK_DISPATCH_ENV_ARM, __VA_ARGS__) }     \
  } while (0)
#define SGK_DISPATCH_ENV_LAYOUT(ENVID, LAYOUT, ...)    \
  do {                                                 \
    if ((LAYOUT) == SGK_LAYOUT_COMPACT) {              \
      constexpr int L = SGK_LAYOUT_COMPACT;            \
      SGK_DISPATCH_ENV(ENVID, __VA_ARGS__);            \
    } else {                                           \
      constexpr int L = SGK_LAYOUT_PITCHED;            \
      SGK_DISPATCH_ENV(ENVID, __VA_ARGS__);            \
    }                                                  \
  } while (0)
