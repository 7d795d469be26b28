// The SPLIT instantiations of k_gcn_layer_ps (plain eval layer on the bf16 matrix path) as a translation unit of their own: build.py
// compiles this file without packed fp32 vector instructions (FILE_FLAGS: target feature -packed-fp32-ops), which return wrong
// results now and then when they run on a SIMD beside v_mfma_f32_32x32x16_bf16 (gcn_layer_ps.hip, in front of ps_split_kernel;
// DESIGN_NOTES 9.8), and then checks the object it made: bf16 MFMAs in it and no v_pk_*_f32, or the build fails.
// (A target("no-packed-fp32-ops") attribute on this unit's functions does the same but keeps the device library's functions --
// __ockl_mul24_i32 inside the tile loop among them -- from being inlined: 20 calls per kernel.  Hence the flag.)
#define EG_PS_SPLIT_TU
#include "gcn_layer_ps.hip"
