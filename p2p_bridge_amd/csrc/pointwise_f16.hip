// pointwise_f16.hip -- pw_wide_kernel (pw_wide.h) in the f16x3 arithmetic: the narrow layers (cin or cout < 128) on the 16-bit
// matrix pipe, reading the split pack of pointwise_split.hip; and its GATHER form, the last layer of a set abstraction on the
// grouped tensor without building it (p2pb_pointwise_conv_pool_gather).
#include "pw_wide.h"

int pw_wide_f16_launch(const PwArgs &a) { return pw_wide_form<SPLIT_F16X3>(a); }

// always transform + statistics; the neighbourhoods as groups of 8 lanes (u = 32) or by the per-row ladder. (The global pool,
// PG = 32, has no gathered form: a set abstraction pools neighbourhoods.)
int pw_gather_launch(const PwArgs &a, const PwGather &gat) {
  return pw_for_mt(a.cout, [&](auto MT) {
    return for_flag(pool_lanes(a.pool_u) == 8, [&](auto G8) {
      return pw_wide_go<MT(), true, true, (G8() ? 8 : 1), SPLIT_F16X3, true>(a, gat);
    });
  });
}
