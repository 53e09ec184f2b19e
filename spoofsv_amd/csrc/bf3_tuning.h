// Per-tile decision tables of the split-MFMA convolution kernels (conv_nn.hip), one place; each comment says which measurement chose the entry.
// None changes results beyond fp32 summation order.  (Settled either / or choices are plain code at their sites; the alternatives that lost are
// recorded in DESIGN_HISTORY.md and profiles/, not kept in the tree.)
#pragma once

#define SSV_NN_XBUF(KT, WM, NT) (!((KT) == 3 && (NT) == 6))   // input rows by buffer loads (ssv_buf) or through pointers: in-step, per tile -- the k = 1
                                                             // tiles are 5-12 % faster with buffer loads, the 96-column k = 3 tiles 4-6 % with pointers, the rest equal

constexpr int SSV_NN_HALO_SMALL = 16;   // k = 3 layers whose taps span at most this many columns run the narrow-halo instantiation

// waves per SIMD the register allocation must leave room for (the second __launch_bounds__ argument).  Round 5: the 128 x 112 k = 3 tile with the
// 16-column halo at THREE (168 VGPRs, 6 spilled, three workgroups per CU instead of two): 177.6 -> 170.4 us in-step over its ten launches.
// (The same for the 128 x 96 tile: 32 spilled, 63.2 -> 70.3 us; the 64 x 96 tile at four, 128 VGPRs: 47.6 -> 49.5 us.  Not kept.)
#define SSV_NNB_WAVES(KT, WM, NT, EPI, HW) \
  (((KT) == 1 && (WM) == 2 && (NT) == 4 && (EPI) == 0) || ((KT) == 3 && (WM) == 2 && (NT) == 7 && (EPI) == 0 && (HW) == 16) ? 3 : 2)
