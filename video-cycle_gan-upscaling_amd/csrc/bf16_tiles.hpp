// bf16-storage kernels (configs C3-C5 of BASELINE.json): activations bf16 NHWC, weights bf16 packed
// [tap][out-channel][in-channel], fp32 accumulation on v_mfma_f32_32x32x16_bf16, fp32 epilogue.
//
// Why NHWC here while the fp32 path is NCHW: the bf16 MFMA takes 8 consecutive k per lane, and k of the
// implicit GEMM is the input channel -- with channels innermost one lane's operand fragment is ONE 16-byte LDS
// read, and a pixel's 64 channels are one 128-byte line in HBM.
//
// Reference ops served: Conv2D 3x3 'same' of residual_block / prefinal conv (upscaling/upscaler/model.py:19,22,283)
// with the inference-mode BatchNormalization folded into a per-channel scale/shift (model.py:20,23,284),
// PReLU (model.py:21) and the block's Add (model.py:25,285) fused into the epilogue.
//
// This header holds what more than one kernel family uses; a family's constants, parameter struct, kernels, launch helpers and
// C entry points live together in its own file: bf16_layout.hip (layout / pack helpers, PReLU backward), bf16_conv3x3_3ch.hip (the
// trunk, v1 and v2, and the convolutions on three input channels, gates included: one file, for the reason given at its top),
// bf16_convt3x3.hip (the up-sampling transposed convolution) and bf16_conv9x9_to3.hip (the final convolution).
#pragma once
#include "vcg_common.hpp"

namespace {

__device__ __forceinline__ f32x16 mfma_bf16(bf16x8 a, bf16x8 b, f32x16 c) {
    // lane l (r = l&31, h = l>>5): A[row r][k = 8h+j], B[k = 8h+j][col r], j = 0..7; D as the f32 form
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// one 16-byte operand fragment (8 bf16) through a range-checked descriptor: VCG_OOB reads as zeros (the generic kernels of bf16_gconv.hip
// and the inception block's 1x1 kernels of bf16_incep.hip)
__device__ __forceinline__ bf16x8 ld_frag(vcg_rsrc r, unsigned off) {
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
}

// A 32x32 MFMA tile leaves lane (column r, half hh) with rows 8g + 4hh + {0..3} in register group g; v_permlane32_swap between the groups
// (2q, 2q+1) of the two half-waves turns that into 8 consecutive rows 16q + 8hh + {0..7} in v: with rows = output channels, one 16-byte
// NHWC store per q.  Every lane of the wave must call it.  (The epilogues of bf16_gconv.hip, bf16_conv3x3_3ch.hip and bf16_convt3x3.hip
// spell the same four swaps out in place: routed through this function the generic kernels' schedule changed, scripts/device_isa.py.)
__device__ __forceinline__ void acc_channels8(const f32x16& acc, int q, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float lo = acc[8 * q + j], hi = acc[8 * q + 4 + j];
        swap32(lo, hi);
        v[j] = lo;
        v[4 + j] = hi;
    }
}

// The 6 + 2-wave skeleton of conv3x3_c64_bf16_kernel (bf16_conv3x3_3ch.hip, where it is described), shared by conv_c3to64_bf16_kernel and
// convt3x3_c64_bf16_kernel: 12x32-pixel tiles, 128-byte pixel rows, the 3x3 weights of one 64-channel output block resident in LDS
constexpr int NCW = 6, NLW = 2;             // compute / loader waves
constexpr int TR = 2 * NCW, TC = 32, HR = TR + 2, HC = TC + 2;
constexpr int ROWB = HC * 128;              // bytes per halo row
constexpr int WB = 9 * 64 * 128;            // 73728
constexpr int NT = (NCW + NLW) * 64;

// Several workgroups write different 128-byte channel blocks of the SAME pixels (cout = 64 nblk): mapped so that the nblk workgroups of one
// tile stream sit on ONE XCD (workgroups b and b + 8 share an XCD under round-robin placement -- speed only, never correctness) and run side by
// side, their pieces of a pixel's 128 nblk bytes meet in that XCD's L2 and leave it together.  An experiment (xcd_group = 1, which no
// caller sets any more), measured neutral (profiles/r03_xcd_group_ab.txt): convT 389 vs 387 us, the final-conv data gradient 717 vs 712 us
// at C3's shard -- the default is the plain b % nblk mapping.
__device__ __forceinline__ void block_and_stream(int nblk, int xcd_group, int& cb, int& wg) {
    const int b = blockIdx.x;
    if (xcd_group && gridDim.x % (8 * nblk) == 0) {
        const int slot = b >> 3;
        cb = slot % nblk;
        wg = (slot / nblk) * 8 + (b & 7);
    } else {
        cb = b % nblk;
        wg = b / nblk;
    }
}

}  // namespace
