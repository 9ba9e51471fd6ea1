// conv3d_bf16x6.hip -- the bf16x6 instantiations (conv_math = bf16x6: three bf16 terms per operand, six products) of the
// split-operand dense and compact kernels, in an object of their own so that they compile beside the default arithmetic's
// (conv3d.hip, which calls these two functions when p2pb_set_split_terms selects them).
#include "conv3d_compact.h"

int conv3d_bf16x6_split(int r, int mt, const ConvArgs &a) { return conv_split_launch<SPLIT_BF16X6>(r, mt, a); }
int conv3d_bf16x6_compact(int r, const ConvArgs &a) { return conv_compact_launch<SPLIT_BF16X6>(r, a); }
