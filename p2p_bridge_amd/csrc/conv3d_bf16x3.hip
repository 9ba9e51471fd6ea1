// conv3d_bf16x3.hip -- the bf16x3 instantiations of the split-operand dense kernel: the arithmetic of the training data gradient
// (p2p_bridge_amd/dense.py), which launches the plain form only -- channel-major, no operand transform, no lists. An object of
// its own so that it compiles beside the other arithmetics' (conv3d.hip calls it when p2pb_set_split_terms selects it).
#include "conv3d_split.h"

int conv3d_bf16x3_split(int r, int mt, const ConvArgs &a) { return conv_split_launch<SPLIT_BF16X3>(r, mt, a); }
