"""The conv dispatch case table, its input generators and its reference.

bnn_conv2d_fwd / _bwd_data / _bwd_filter choose among 75 kernel template instances by shape and by
three process-global switches.  Each case below is a shape plus switch settings and the instance
names (bnn_conv_kernel's answer) it reaches for the three ops.  MAIN was found by searching with
that query on the CPU: the cheapest shape per (instance, schedule), preferring ragged edges (N not
a multiple of 8 and above one workgroup's samples, Co not a multiple of 8, OH*OW not a multiple of
16, OW not a multiple of 8, C*KH*KW not a multiple of 16, H != W), then a greedy cover.  GEOMETRY
is what only the generic kernels take; NONSQUARE is KH != KW through a tiled, an MFMA and the
generic kernel.  The table runs with the popcount engine off (tests/test_gpu_conv_popc.py has it).

The reference is oracle.bnn_np.conv2d_forward / conv2d_backward (float64), which binarises the
input unless C == 3 (the reference module's rule), so a case has binarize == (C != 3).

Shared by test_conv_dispatch.py (CPU: the table covers the dispatch) and
test_gpu_conv_dispatch.py (the kernels compute what the reference computes).
"""
import collections

import numpy as np

from oracle import bnn_np as O

Case = collections.namedtuple(
    "Case", "N C H W Co KH KW stride pad dil groups bias binarize mfma c1f fwd data filt")
C = Case

OPS = ("fwd", "data", "filt")

# (N, C, H, W, Co, KH, KW, stride, pad, dil, groups, bias, binarize, mfma mode, c1 filter,
#  forward instance, backward-data instance, backward-filter instance)
MAIN = [
    # mode 0: the VALU LDS-tiled kernels and the generic ones
    C(3, 1, 3, 4, 12, 3, 5, 1, 2, 1, 1, True, 1, 0, 1, "conv_fwd_bin_tile_k<16>", "conv_bwd_data_tile_k<8>", "conv_bwd_filter_tile_k<16>"),
    C(3, 1, 4, 5, 33, 3, 3, 1, 1, 1, 1, False, 1, 0, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_tile_k<8>", "conv_bwd_filter_tile_k<64>"),
    C(3, 3, 4, 6, 17, 1, 1, 1, 0, 1, 1, True, 0, 0, 1, "conv_fwd_f32_tile_k<32>", "conv_bwd_data_tile_k<8>", "conv_bwd_filter_tile_k<32>"),
    C(3, 12, 4, 3, 1, 5, 5, 1, 1, 1, 1, False, 1, 0, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_tile_k<16>", "conv_bwd_filter_tile_k<8>"),
    C(9, 17, 3, 3, 3, 1, 1, 1, 0, 1, 1, False, 1, 0, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_tile_k<32>", "conv_bwd_filter_tile_k<8>"),
    C(9, 64, 6, 5, 33, 7, 7, 1, 2, 1, 1, True, 1, 0, 1, "conv_fwd_k", "conv_bwd_data_k", "conv_bwd_filter_k"),
    # mode 1 (the default): int8-MFMA / dot4 forward, bf16x3 backward, f32-MFMA filter for an fp32 input
    C(9, 1, 3, 10, 1, 3, 3, 1, 2, 1, 1, True, 1, 1, 1, "conv_fwd_bin_c1_k<8,1>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_c1_k<3,3>"),
    C(3, 1, 5, 17, 1, 5, 1, 1, 0, 1, 1, True, 1, 1, 0, "conv_fwd_bin_c1_k<8,1>", "conv_bwd_data_bf3_k<1,1> rowt=0 ipb=8", "conv_bwd_filter_bf3_k<1,1> WT=1 KS=8 ipb=8"),
    C(3, 1, 9, 18, 1, 3, 5, 1, 0, 1, 1, True, 1, 1, 0, "conv_fwd_bin_c1_k<8,2>", "conv_bwd_data_bf3_k<1,2> rowt=0 ipb=8", "conv_bwd_filter_bf3_k<1,1> WT=1 KS=8 ipb=8"),
    C(9, 1, 10, 33, 1, 5, 1, 1, 0, 1, 1, True, 1, 1, 1, "conv_fwd_bin_c1_k<8,1>", "conv_bwd_data_bf3_k<1,4> rowt=0 ipb=8", "conv_bwd_filter_bf3_k<1,1> WT=1 KS=8 ipb=8"),
    C(3, 1, 28, 3, 1, 3, 3, 1, 0, 1, 1, True, 1, 1, 0, "conv_fwd_bin_c1_k<8,1>", "conv_bwd_data_bf3_k<1,4> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<1,1> WT=1 KS=8 ipb=8"),
    C(3, 1, 40, 5, 1, 3, 3, 1, 1, 1, 1, False, 1, 1, 0, "conv_fwd_bin_c1_k<8,1>", "conv_bwd_data_bf3_k<1,8> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<1,1> WT=1 KS=8 ipb=8"),
    C(3, 1, 65, 9, 1, 5, 5, 1, 1, 1, 1, True, 1, 1, 0, "conv_fwd_bin_c1_k<8,2>", "conv_bwd_data_mfma_k<1,13>", "conv_bwd_filter_bf3_k<1,1> WT=2 KS=4 ipb=8"),
    C(3, 1, 65, 6, 1, 1, 1, 1, 0, 1, 1, True, 1, 1, 0, "conv_fwd_bin_c1_k<8,1>", "conv_bwd_data_bf3_k<1,16> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<1,1> WT=1 KS=8 ipb=8"),
    C(3, 1, 3, 6, 12, 1, 5, 1, 0, 1, 1, False, 1, 1, 1, "conv_fwd_bin_c1_k<16,2>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<1,1> WT=1 KS=8 ipb=8"),
    C(3, 1, 5, 3, 17, 3, 3, 1, 0, 1, 1, True, 1, 1, 0, "conv_fwd_bin_c1_k<32,1>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<2,1> WT=1 KS=8 ipb=8"),
    C(3, 1, 3, 4, 24, 7, 7, 1, 2, 1, 1, False, 1, 1, 0, "conv_fwd_bin_c1_k<32,2>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<2,1> WT=4 KS=2 ipb=8"),
    C(11, 1, 4, 3, 33, 5, 5, 1, 2, 1, 1, True, 1, 1, 1, "conv_fwd_bin_c1_k<64,2>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<3,1> WT=2 KS=4 ipb=8"),
    C(3, 1, 7, 3, 33, 3, 3, 1, 0, 1, 1, True, 1, 1, 0, "conv_fwd_bin_c1_k<64,1>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<3,1> WT=1 KS=8 ipb=8"),
    C(11, 2, 5, 3, 33, 5, 5, 1, 2, 1, 1, False, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<3,1> WT=4 KS=2 ipb=8"),
    C(9, 2, 7, 5, 33, 7, 7, 1, 1, 1, 1, False, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<3,2> WT=4 KS=2 ipb=8"),
    C(3, 2, 4, 6, 57, 3, 3, 1, 1, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<4,1> WT=2 KS=4 ipb=8"),
    C(3, 2, 6, 3, 57, 1, 1, 1, 0, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<4,1> WT=1 KS=8 ipb=8"),
    C(11, 3, 30, 18, 9, 1, 1, 1, 0, 1, 1, True, 0, 1, 1, "conv_fwd_f32_tile_k<16>", "conv_bwd_data_bf3_k<1,8> rowt=0 ipb=8", "conv_bwd_filter_mfma_k<1> WT=1 KS=4"),
    C(3, 3, 3, 4, 33, 1, 1, 1, 0, 1, 1, True, 0, 1, 1, "conv_fwd_f32_tile_k<64>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_mfma_k<2> WT=2 KS=2"),
    C(11, 5, 6, 3, 1, 3, 3, 1, 0, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<1,2> WT=2 KS=4 ipb=8"),
    C(3, 5, 14, 3, 3, 5, 5, 1, 1, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_bf3_k<1,2> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<1,1> WT=8 KS=1 ipb=8"),
    C(3, 5, 3, 5, 17, 7, 7, 1, 2, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<32>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<2,2> WT=8 KS=1 ipb=8"),
    C(3, 5, 3, 9, 33, 5, 5, 1, 1, 1, 1, False, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<3,1> WT=8 KS=1 ipb=8"),
    C(3, 5, 10, 3, 33, 3, 3, 1, 1, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_bf3_k<1,2> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<3,2> WT=2 KS=4 ipb=8"),
    C(11, 5, 3, 7, 57, 3, 3, 1, 2, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<4,2> WT=2 KS=4 ipb=8"),
    C(9, 7, 3, 3, 1, 3, 3, 1, 2, 1, 1, False, 1, 1, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<1,1> WT=4 KS=2 ipb=8"),
    C(3, 7, 7, 3, 17, 7, 7, 1, 2, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<32>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<2,4> WT=8 KS=1 ipb=8"),
    C(11, 7, 4, 5, 57, 3, 3, 1, 2, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<4,1> WT=4 KS=2 ipb=8"),
    C(11, 7, 5, 3, 57, 5, 5, 1, 2, 1, 1, False, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<4,2> WT=8 KS=1 ipb=8"),
    C(9, 8, 5, 3, 17, 5, 1, 1, 0, 1, 1, False, 1, 1, 1, "conv_fwd_bin_tile_k<32>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<2,2> WT=2 KS=4 ipb=8"),
    C(3, 8, 4, 6, 57, 3, 3, 1, 1, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<4,2> WT=4 KS=2 ipb=8"),
    C(11, 12, 4, 6, 1, 5, 5, 1, 2, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<1,4> WT=8 KS=1 ipb=8"),
    C(3, 17, 23, 5, 1, 5, 1, 1, 0, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_bf3_k<2,4> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<1,2> WT=4 KS=2 ipb=8"),
    C(3, 17, 28, 17, 1, 1, 1, 1, 0, 1, 1, False, 1, 1, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_bf3_k<2,4> rowt=0 ipb=8", "conv_bwd_filter_bf3_k<1,1> WT=2 KS=4 ipb=8"),
    C(3, 17, 40, 3, 1, 3, 3, 1, 1, 1, 1, False, 1, 1, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_bf3_k<2,8> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<1,2> WT=8 KS=1 ipb=8"),
    C(3, 17, 6, 3, 17, 5, 1, 1, 0, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<32>", "conv_bwd_data_bf3_k<2,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<2,2> WT=4 KS=2 ipb=8"),
    C(3, 17, 3, 4, 33, 3, 3, 1, 0, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_bf3_k<2,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<3,2> WT=8 KS=1 ipb=8"),
    C(3, 20, 6, 17, 1, 1, 5, 1, 0, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_bf3_k<2,1> rowt=0 ipb=8", "conv_bwd_filter_bf3_k<1,2> WT=4 KS=2 ipb=8"),
    C(3, 20, 9, 7, 3, 1, 1, 1, 0, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_bf3_k<2,2> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<1,1> WT=2 KS=4 ipb=8"),
    C(9, 20, 70, 3, 3, 5, 1, 1, 0, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_bf3_k<2,16> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<1,2> WT=4 KS=2 ipb=8"),
    C(3, 20, 5, 33, 5, 1, 1, 1, 0, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_bf3_k<2,2> rowt=0 ipb=8", "conv_bwd_filter_bf3_k<1,1> WT=2 KS=4 ipb=8"),
    C(17, 24, 3, 3, 1, 5, 5, 1, 1, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_bf3_k<2,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<1,8> WT=8 KS=1 ipb=8"),
    C(11, 24, 3, 7, 17, 1, 5, 1, 0, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<32>", "conv_bwd_data_bf3_k<2,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<2,1> WT=8 KS=1 ipb=8"),
    C(3, 24, 3, 6, 57, 1, 5, 1, 0, 1, 1, False, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_bf3_k<2,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<4,1> WT=8 KS=1 ipb=8"),
    C(11, 24, 3, 9, 57, 5, 5, 1, 1, 1, 1, False, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_bf3_k<2,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<4,8> WT=8 KS=1 ipb=8"),
    C(9, 32, 4, 3, 17, 1, 1, 1, 0, 1, 1, True, 1, 1, 1, "conv_fwd_i8mfma_k<2>", "conv_bwd_data_bf3_k<2,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<2,1> WT=2 KS=4 ipb=8"),
    C(11, 33, 3, 4, 17, 5, 5, 1, 2, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<32>", "conv_bwd_data_tile_k<64>", "conv_bwd_filter_bf3_k<2,8> WT=8 KS=1 ipb=8"),
    C(3, 33, 5, 4, 33, 3, 3, 1, 2, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_tile_k<64>", "conv_bwd_filter_bf3_k<3,4> WT=8 KS=1 ipb=8"),
    C(3, 33, 9, 3, 57, 3, 3, 1, 2, 1, 1, True, 1, 1, 1, "conv_fwd_bin_tile_k<64>", "conv_bwd_data_tile_k<64>", "conv_bwd_filter_bf3_k<4,4> WT=8 KS=1 ipb=8"),
    C(11, 48, 4, 3, 33, 3, 5, 1, 2, 1, 1, True, 1, 1, 1, "conv_fwd_i8mfma_k<4>", "conv_bwd_data_tile_k<64>", "conv_bwd_filter_bf3_k<3,8> WT=8 KS=1 ipb=8"),
    # mode 2: the f32-MFMA backward data kernel, and the f32-MFMA filter kernel for a binarised input
    C(17, 1, 6, 4, 1, 5, 5, 1, 2, 1, 1, True, 1, 2, 1, "conv_fwd_bin_c1_k<8,2>", "conv_bwd_data_mfma_k<1,1>", "conv_bwd_filter_c1_k<5,5>"),
    C(3, 1, 7, 14, 1, 1, 5, 1, 0, 1, 1, False, 1, 2, 1, "conv_fwd_bin_c1_k<8,2>", "conv_bwd_data_mfma_k<1,2>", "conv_bwd_filter_mfma_k<1> WT=1 KS=4"),
    C(3, 1, 13, 10, 1, 3, 5, 1, 0, 1, 1, True, 1, 2, 1, "conv_fwd_bin_c1_k<8,2>", "conv_bwd_data_mfma_k<1,4>", "conv_bwd_filter_mfma_k<1> WT=1 KS=4"),
    C(3, 1, 65, 4, 1, 1, 1, 1, 0, 1, 1, True, 1, 2, 1, "conv_fwd_bin_c1_k<8,1>", "conv_bwd_data_mfma_k<1,8>", "conv_bwd_filter_mfma_k<1> WT=1 KS=4"),
    C(3, 1, 129, 7, 1, 1, 1, 1, 0, 1, 1, False, 1, 2, 1, "conv_fwd_bin_c1_k<8,1>", "conv_bwd_data_mfma_k<1,16>", "conv_bwd_filter_mfma_k<1> WT=1 KS=4"),
    C(3, 1, 3, 5, 9, 1, 1, 1, 0, 1, 1, True, 1, 2, 1, "conv_fwd_bin_c1_k<16,1>", "conv_bwd_data_mfma_k<1,1>", "conv_bwd_filter_mfma_k<1> WT=1 KS=4"),
    C(3, 1, 5, 3, 57, 1, 1, 1, 0, 1, 1, True, 1, 2, 1, "conv_fwd_bin_c1_k<64,1>", "conv_bwd_data_mfma_k<1,1>", "conv_bwd_filter_mfma_k<1> WT=4 KS=1"),
    C(3, 3, 5, 9, 1, 7, 7, 1, 2, 1, 1, True, 0, 2, 1, "conv_fwd_f32_tile_k<8>", "conv_bwd_data_mfma_k<1,1>", "conv_bwd_filter_mfma_k<4> WT=4 KS=1"),
    C(11, 7, 6, 7, 1, 9, 9, 1, 2, 1, 1, False, 1, 2, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_mfma_k<1,1>", "conv_bwd_filter_mfma_k<13> WT=4 KS=1"),
    C(3, 16, 3, 4, 1, 1, 1, 1, 0, 1, 1, True, 1, 2, 1, "conv_fwd_i8mfma_k<1>", "conv_bwd_data_mfma_k<1,1>", "conv_bwd_filter_mfma_k<1> WT=1 KS=4"),
    C(3, 17, 4, 6, 1, 5, 5, 1, 2, 1, 1, True, 1, 2, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_mfma_k<2,1>", "conv_bwd_filter_mfma_k<8> WT=4 KS=1"),
    C(3, 17, 4, 17, 3, 1, 1, 1, 0, 1, 1, True, 1, 2, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_mfma_k<2,2>", "conv_bwd_filter_mfma_k<1> WT=2 KS=2"),
    C(3, 17, 20, 13, 3, 1, 1, 1, 0, 1, 1, False, 1, 2, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_mfma_k<2,8>", "conv_bwd_filter_mfma_k<1> WT=2 KS=2"),
    C(3, 20, 7, 6, 1, 7, 7, 1, 1, 1, 1, True, 1, 2, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_mfma_k<2,1>", "conv_bwd_filter_mfma_k<16> WT=4 KS=1"),
    C(3, 20, 17, 33, 3, 5, 1, 1, 0, 1, 1, True, 1, 2, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_mfma_k<2,16>", "conv_bwd_filter_mfma_k<2> WT=4 KS=1"),
    C(3, 20, 23, 6, 5, 1, 1, 1, 0, 1, 1, False, 1, 2, 1, "conv_fwd_bin_tile_k<8>", "conv_bwd_data_mfma_k<2,4>", "conv_bwd_filter_mfma_k<1> WT=2 KS=2"),
]

GEN = ("conv_fwd_k", "conv_bwd_data_k", "conv_bwd_filter_k")

# what only the generic kernels take: each property alone, then combined
GEOMETRY = [
    C(3, 4, 9, 7, 6, 3, 3, 2, 1, 1, 1, True, 1, 1, 1, *GEN),        # stride 2
    C(2, 5, 11, 10, 3, 3, 3, 3, 0, 1, 1, False, 1, 1, 1, *GEN),     # stride 3
    C(3, 4, 9, 8, 5, 3, 3, 1, 2, 2, 1, True, 1, 1, 1, *GEN),        # dilation 2
    C(3, 6, 7, 8, 10, 3, 3, 1, 1, 1, 2, True, 1, 1, 1, *GEN),       # groups 2
    C(2, 6, 8, 7, 6, 3, 3, 1, 1, 1, 6, True, 1, 1, 1, *GEN),        # depthwise: groups = C = Co
    C(3, 2, 6, 5, 3, 3, 3, 1, 3, 1, 1, True, 1, 1, 1,               # pad > K - 1
      "conv_fwd_k", "conv_bwd_data_k", "conv_bwd_filter_mfma_k<1> WT=2 KS=2"),
    C(2, 65, 5, 4, 5, 3, 3, 1, 1, 1, 1, True, 1, 1, 1,              # C > 64
      "conv_fwd_k", "conv_bwd_data_k", "conv_bwd_filter_bf3_k<1,8> WT=8 KS=1 ipb=8"),
    C(2, 2, 6, 5, 65, 3, 3, 1, 1, 1, 1, True, 1, 1, 1,              # Co > 64
      "conv_fwd_k", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_k"),
    C(2, 3, 6, 5, 65, 3, 3, 1, 1, 1, 1, True, 0, 1, 1,              # Co > 64, fp32 input
      "conv_fwd_k", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_k"),
    C(3, 3, 9, 8, 5, 3, 3, 2, 1, 1, 1, True, 0, 1, 1, *GEN),        # stride 2, fp32 input
    C(3, 4, 11, 9, 6, 3, 5, 2, 2, 2, 2, True, 1, 1, 1, *GEN),       # stride, pad, dilation, groups, KH != KW
    C(2, 3, 10, 9, 6, 5, 3, 3, 1, 1, 3, False, 0, 1, 1, *GEN),      # stride 3, groups 3, fp32 input, KH != KW
    C(2, 66, 7, 6, 4, 3, 3, 2, 3, 1, 2, True, 1, 1, 1, *GEN),       # C > 64, stride 2, pad > K - 1, groups 2
    C(3, 1, 2, 2, 2, 3, 3, 2, 1, 1, 1, True, 1, 1, 1, *GEN),        # an input smaller than the kernel, padded
]

# KH != KW in both orders through a tiled (mode 0), an MFMA (modes 1, 2) and the generic kernel
NONSQUARE = [
    C(9, 5, 7, 6, 9, 1, 5, 1, 0, 1, 1, True, 1, 0, 1, "conv_fwd_bin_tile_k<16>", "conv_bwd_data_tile_k<8>", "conv_bwd_filter_tile_k<16>"),
    C(9, 16, 7, 6, 57, 1, 5, 1, 0, 1, 1, True, 1, 1, 1, "conv_fwd_i8mfma_k<4>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<4,2> WT=4 KS=2 ipb=8"),
    C(9, 12, 7, 6, 20, 1, 5, 1, 0, 1, 1, False, 1, 2, 1, "conv_fwd_bin_tile_k<32>", "conv_bwd_data_mfma_k<1,1>", "conv_bwd_filter_mfma_k<2> WT=4 KS=1"),
    C(3, 4, 9, 8, 6, 1, 5, 2, 0, 1, 1, True, 1, 1, 1, *GEN),
    C(9, 5, 7, 6, 9, 5, 1, 1, 0, 1, 1, True, 1, 0, 1, "conv_fwd_bin_tile_k<16>", "conv_bwd_data_tile_k<8>", "conv_bwd_filter_tile_k<16>"),
    C(9, 16, 7, 6, 57, 5, 1, 1, 0, 1, 1, True, 1, 1, 1, "conv_fwd_i8mfma_k<4>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<4,2> WT=4 KS=2 ipb=8"),
    C(9, 12, 7, 6, 20, 5, 1, 1, 0, 1, 1, False, 1, 2, 1, "conv_fwd_bin_tile_k<32>", "conv_bwd_data_mfma_k<1,1>", "conv_bwd_filter_mfma_k<2> WT=4 KS=1"),
    C(3, 4, 9, 8, 6, 5, 1, 2, 0, 1, 1, True, 1, 1, 1, *GEN),
    C(9, 5, 7, 6, 9, 3, 5, 1, 1, 1, 1, True, 1, 0, 1, "conv_fwd_bin_tile_k<16>", "conv_bwd_data_tile_k<8>", "conv_bwd_filter_tile_k<16>"),
    C(9, 16, 7, 6, 57, 3, 5, 1, 2, 1, 1, True, 1, 1, 1, "conv_fwd_i8mfma_k<4>", "conv_bwd_data_bf3_k<1,1> rowt=1 ipb=8", "conv_bwd_filter_bf3_k<4,2> WT=8 KS=1 ipb=8"),
    C(9, 12, 7, 6, 20, 3, 5, 1, 1, 1, 1, False, 1, 2, 1, "conv_fwd_bin_tile_k<32>", "conv_bwd_data_mfma_k<1,1>", "conv_bwd_filter_mfma_k<8> WT=4 KS=1"),
    C(3, 4, 9, 8, 6, 3, 5, 2, 2, 1, 1, True, 1, 1, 1, *GEN),
]

CASES = MAIN + GEOMETRY + NONSQUARE


def case_id(c):
    s = f"n{c.N}c{c.C}h{c.H}w{c.W}o{c.Co}k{c.KH}x{c.KW}"
    if (c.stride, c.pad, c.dil, c.groups) != (1, 0, 1, 1):
        s += f"s{c.stride}p{c.pad}d{c.dil}g{c.groups}"
    return s + f"-m{c.mfma}f{c.c1f}" + ("" if c.binarize else "-fp32") + ("-b" if c.bias else "")


def base(name):
    """The template instance of a query answer (schedule suffixes dropped)."""
    return name.split(" ")[0]


def schedule(name):
    """The schedule suffixes of a query answer as a dict: {"rowt": 1, "ipb": 8} ..."""
    return {k: int(v) for k, v in (t.split("=") for t in name.split(" ")[1:])}


def out_hw(c):
    return ((c.H + 2 * c.pad - c.dil * (c.KH - 1) - 1) // c.stride + 1,
            (c.W + 2 * c.pad - c.dil * (c.KW - 1) - 1) // c.stride + 1)


def set_switches(lib, c):
    """Set the case's switches; returns the popcount setting found, for restore_switches."""
    popc = lib.bnn_conv_set_popc(-1)
    lib.bnn_conv_set_mfma(c.mfma)
    lib.bnn_conv_set_c1_filter(c.c1f)
    lib.bnn_conv_set_popc(0)
    return popc


def restore_switches(lib, popc):
    """The defaults every other test file assumes: MFMA mode 1, c1 filter on, popcount as found."""
    lib.bnn_conv_set_mfma(1)
    lib.bnn_conv_set_c1_filter(1)
    lib.bnn_conv_set_popc(popc)


def query(lib, c):
    """bnn_conv_kernel's answers for the three ops under the switches currently set."""
    return tuple(lib.bnn_conv_kernel(op, int(c.binarize), c.N, c.C, c.H, c.W, c.Co, c.KH, c.KW, c.stride, c.pad,
                                     c.dil, c.groups).decode() for op in range(3))


def instances(lib, op):
    """Every instance the op can launch (bnn_conv_kernel_at until the empty string)."""
    out = []
    while True:
        name = lib.bnn_conv_kernel_at(op, len(out))
        if not name:
            return out
        out.append(name.decode())


def is_mma(name):
    """bf16x3 or f32-MFMA backward kernels: the ones the one-hot inputs are for."""
    return "_bf3_k<" in name or "_mfma_k<" in name


# ------------------------------------------------------------------------------------------- inputs
def _rng(c, kind):
    return np.random.default_rng([int(v) for v in c[:15]] + [kind])


def _shapes(c):
    oh, ow = out_hw(c)
    return (c.N, c.C, c.H, c.W), (c.Co, c.C // c.groups, c.KH, c.KW), (c.N, c.Co, oh, ow)


def _latent(rng, ws):
    w = rng.uniform(-1, 1, ws)
    w = np.where(w == 0, 0.5, w)
    return np.where(rng.random(ws) < 0.1, 0, w).astype(np.float32)


def _real_x(rng, xs):
    return np.where(rng.random(xs) < 0.2, 0, rng.standard_normal(xs)).astype(np.float32)


def real_inputs(c):
    """The parity tests' inputs: standard normal x with ~20 % zeros, uniform latent weight with
    ~10 % zeros, standard normal bias and dy."""
    rng = _rng(c, 0)
    xs, ws, ys = _shapes(c)
    b = rng.standard_normal(c.Co).astype(np.float32) if c.bias else None
    return _real_x(rng, xs), _latent(rng, ws), b, rng.standard_normal(ys).astype(np.float32)


def exact_inputs(c):
    """Inputs under which every partial sum of y, dx, dw and db, in any order, is exact in fp32:
    dy integers in [-8, 8], the weight +-1 / 0 after sign(), x +-1 / 0 after sign() (or multiples
    of 1/4 in [-4, 4] where it is not binarised), the bias multiples of 1/8.  Asserted here from
    the reference's own sum of absolute terms: sum|terms| / lsb < 2^24 for every output element."""
    rng = _rng(c, 1)
    xs, ws, ys = _shapes(c)
    x = _real_x(rng, xs) if c.binarize else (rng.integers(-16, 17, xs) / 4).astype(np.float32)
    w = _latent(rng, ws)
    b = (rng.integers(-16, 17, c.Co) / 8).astype(np.float32) if c.bias else None
    dy = rng.integers(-8, 9, ys).astype(np.float32)
    # sums of absolute terms through the same reference: |x_used|, |sign(w)| (= its own sign), |dy|
    geo = (c.stride, c.pad, c.dil, c.groups)
    xa = np.abs(O.binarize(x) if c.binarize else x)
    wa = np.abs(O.binarize(w))
    cols, _ = O.im2col(xa.astype(np.float64), c.KH, c.KW, c.stride, c.pad, c.dil)
    kg, cog = (c.C // c.groups) * c.KH * c.KW, c.Co // c.groups
    ya = max(float((wa[g * cog:(g + 1) * cog].reshape(cog, kg).astype(np.float64) @ cols[:, g * kg:(g + 1) * kg]).max())
             for g in range(c.groups)) + (float(np.abs(b).max()) if c.bias else 0.0)
    dxa, dwa, dba = O.conv2d_backward(xa, wa, np.abs(dy), *geo)
    x_lsb = 1.0 if c.binarize else 0.25
    for what, amax, lsb in (("y", ya, 0.125 if c.bias else x_lsb), ("dx", dxa.max(), 1.0), ("dw", dwa.max(), x_lsb),
                            ("db", dba.max(), 1.0)):
        assert amax / lsb < 2 ** 24, (what, amax, lsb)
    return x, w, b, dy


def _full_mantissa(rng, shape):
    """Standard normal times 2^k, k uniform in [-20, 20] per element: full 24-bit mantissas over 40
    binades (the scaling is exact)."""
    return np.ldexp(rng.standard_normal(shape).astype(np.float32), rng.integers(-20, 21, shape)).astype(np.float32)


def onehot_dx_inputs(c):
    """dx becomes +- a shifted copy of one dy plane: the latent weight is zero except one tap per
    input channel, all in one output channel, so every dx element is one product dy * (+-1) plus
    exact zeros -- the kernel must return dy's 24 bits (all three bf16 terms of the bf16x3 split)."""
    assert c.groups == 1
    rng = _rng(c, 2)
    xs, ws, ys = _shapes(c)
    w = np.zeros(ws, np.float32)
    co = int(rng.integers(c.Co))
    for ci in range(c.C):
        w[co, ci, rng.integers(c.KH), rng.integers(c.KW)] = rng.choice([-1, 1]) * rng.uniform(0.1, 1)
    b = np.zeros(c.Co, np.float32) if c.bias else None
    return _real_x(rng, xs), w, b, _full_mantissa(rng, ys)


def onehot_dw_inputs(c):
    """dw becomes +- single dy elements: x is zero except one pixel per channel in sample 0, so every
    dw element is dy[0, co, oh, ow] * (+-1) (or 0 where the tap falls outside the output)."""
    assert c.groups == 1
    rng = _rng(c, 3)
    xs, ws, ys = _shapes(c)
    x = np.zeros(xs, np.float32)
    for ci in range(c.C):
        x[0, ci, rng.integers(c.H), rng.integers(c.W)] = rng.choice([-1, 1]) * (0.75 if c.binarize else 1.0)
    b = np.zeros(c.Co, np.float32) if c.bias else None
    return x, _latent(rng, ws), b, _full_mantissa(rng, ys)


# ---------------------------------------------------------------------------------------- reference
def reference(c, x, w, b, dy):
    """(y, dx, dw, db) of the float64 oracle, rounded once to fp32."""
    assert c.binarize == O.conv_binarizes_input(x), "the oracle binarises unless C == 3"
    geo = (c.stride, c.pad, c.dil, c.groups)
    y, xu = O.conv2d_forward(x, w, b, *geo)
    return (y,) + O.conv2d_backward(xu, w, dy, *geo)


def first_mismatch(got, want):
    """'' when the arrays are equal, else the first differing index and the two values."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if len(bad) == 0:
        return ""
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} of {got.size} differ; first at {i}: got {got[i]!r}, want {want[i]!r}"
