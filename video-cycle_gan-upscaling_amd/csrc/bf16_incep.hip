// bf16 inference of make_upscaler_incep_resnet (upscaling/upscaler/model.py:443-497, blocks :372-440; train_gan3.py's -gm inc-resnet):
// the 1x1 layers at both ends of an inception block, and the packing that every layer of a block shares.
//
// A block is  m -> { path: [BN -> PReLU -> Conv]+ } -> Concatenate -> Conv 1x1 -> Add(m)  with pre-activation mini-blocks (model.py:372-382).
// In learning phase 0 a BatchNormalization is a per-channel scale / shift, so wherever a convolution's output has ONE consumer, that
// consumer's BN + PReLU runs in the producer's epilogue and the ACTIVATED tensor is the one stored (TF-SAME zero padding of the consumer is
// then zero padding of the activated tensor, as Keras has it).  Only the block input m, read by every path and the Add, is activated on load:
//
//   head  (incep_head_bf16_kernel):  per path p   u_p = prelu_p(scale_p * m + shift_p)  -> bf16 (the MFMA operand)
//                                                 t_p = W_p(1x1, K = 64) u_p            fp32
//                                                 y_p = act(oscale_p * t_p + oshift_p)  -> bf16   (oshift carries the bias; a/1: no act)
//   join  (incep_join_bf16_kernel):  y = m + bias + sum_s W_s(1x1) z_s                  the concatenation [z_a | z_b | z_c] never exists
//
// Both are implicit GEMMs on v_mfma_f32_32x32x16_bf16 in the generic kernels' orientation (bf16_gconv.hip): A = weight fragments (rows =
// output channels), B = 32 consecutive pixels, a lane's B fragment = 8 consecutive channels of ITS pixel = one 16-byte load.  One wave per
// 32-pixel tile; no LDS, no barrier.  The layers between head and join (3x3 / 5x5 / 1xk / kx1) run on the generic kernels themselves
// (vcg_conv2d_nhwc_bf16_fwd_epilogue, bf16_gconv.hip).
//
// Channel padding.  The paths have 19, 25, 32, 48 and 64 channels; a stored tensor and a packed kernel are padded to the next multiple
// of 32 (vcg_incep_padded_channels).  Packed weights are ZERO in the padding, and so are the folded epilogue vectors (vcg_incep_fold), so
// a producer's epilogue computes act(0 * 0 + 0) = +0 for a padded channel of every pixel: the consumer never multiplies a zero weight with
// what an uninitialised buffer held (0 x NaN = NaN in the MFMA).
#include "bf16_tiles.hpp"

namespace {

constexpr int IC_MAXPATHS = 3, IC_MAXSRC = 3;

struct IhPath {
    const float* iscale;    // [64] the path's first BatchNormalization, folded (no bias: m is a stored tensor)
    const float* ishift;
    const float* ialpha;    // [64] its PReLU
    const void* wf;         // fragments [64/16][1][64 lanes] x 16 bytes (32 padded output channels)
    const float* oscale;    // [32] epilogue: y = act(oscale * t + oshift)
    const float* oshift;
    const float* oalpha;    // [32] or null (no activation)
    void* y;                // bf16 NHWC [pixels][32]
};

struct IhParams {
    const void* m;          // bf16 NHWC [pixels][64]
    long pixels;
    int npaths;
    IhPath p[IC_MAXPATHS];
};

__global__ __launch_bounds__(256) void incep_head_bf16_kernel(const IhParams p) {
    const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long tile = (long)blockIdx.x * 4 + wv;
    if (tile * 32 >= p.pixels) return;
    const long P = tile * 32 + r;
    const bool ok = P < p.pixels;
    const vcg_rsrc rm = make_rsrc(p.m, (size_t)p.pixels * 128);
    const unsigned moff = ok ? (unsigned)(P * 128 + 16 * hh) : VCG_OOB;     // (pixels * 128 < 4 GiB: checked by the entry point)
    bf16x8 mv[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) mv[ks] = ld_frag(rm, moff == VCG_OOB ? VCG_OOB : moff + (unsigned)ks * 32u);

    for (int pi = 0; pi < p.npaths; ++pi) {
        const IhPath& pp = p.p[pi];
        const vcg_rsrc rw = make_rsrc(pp.wf, 64 * 32 * 2);
        bf16x8 a[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) a[ks] = ld_frag(rw, (unsigned)(ks * 1024 + lane * 16));
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int c0 = ks * 16 + 8 * hh;
            bf16x8 u;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float t = fmaf((float)mv[ks][j], pp.iscale[c0 + j], pp.ishift[c0 + j]);
                t = t >= 0.f ? t : t * pp.ialpha[c0 + j];
                u[j] = (__bf16)t;
            }
            acc = mfma_bf16(a[ks], u, acc);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int co = 16 * q + 8 * hh;
            float v[8];
            acc_channels8(acc, q, v);
            if (!ok) continue;
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float t = fmaf(v[j], pp.oscale[co + j], pp.oshift[co + j]);
                if (pp.oalpha) t = t >= 0.f ? t : t * pp.oalpha[co + j];
                o[j] = (__bf16)t;
            }
            *(bf16x8*)((__bf16*)pp.y + P * 32 + co) = o;
        }
    }
}

struct IjParams {
    const void* z[IC_MAXSRC];      // bf16 NHWC [pixels][zc[s]]
    const void* wf[IC_MAXSRC];     // fragments [zc[s]/16][2][64 lanes] x 16 bytes: the source's rows of the (1,1,sum zc,64) kernel
    int zc[IC_MAXSRC];             // 32 or 64
    int nsrc;
    const float* bias;             // [64]
    const void* m;                 // bf16 NHWC [pixels][64]: the block input
    void* y;                       // bf16 NHWC [pixels][64]
    long pixels;
};

__global__ __launch_bounds__(256) void incep_join_bf16_kernel(const IjParams p) {
    const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long tile = (long)blockIdx.x * 4 + wv;
    if (tile * 32 >= p.pixels) return;
    const long P = tile * 32 + r;
    const bool ok = P < p.pixels;
    f32x16 acc[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[mb][e] = 0.f;
    for (int s = 0; s < p.nsrc; ++s) {
        const int zc = p.zc[s], ksteps = zc >> 4;
        const vcg_rsrc rz = make_rsrc(p.z[s], (size_t)p.pixels * zc * 2);
        const vcg_rsrc rw = make_rsrc(p.wf[s], (size_t)zc * 64 * 2);
        const unsigned zoff = ok ? (unsigned)(P * zc * 2 + 16 * hh) : VCG_OOB;
        for (int ks = 0; ks < ksteps; ++ks) {
            const bf16x8 b = ld_frag(rz, zoff == VCG_OOB ? VCG_OOB : zoff + (unsigned)ks * 32u);
            const bf16x8 a0 = ld_frag(rw, (unsigned)((ks * 2) * 1024 + lane * 16));
            const bf16x8 a1 = ld_frag(rw, (unsigned)((ks * 2 + 1) * 1024 + lane * 16));
            acc[0] = mfma_bf16(a0, b, acc[0]);
            acc[1] = mfma_bf16(a1, b, acc[1]);
        }
    }
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int co = mb * 32 + 16 * q + 8 * hh;
            float v[8];
            acc_channels8(acc[mb], q, v);
            if (!ok) continue;
            const bf16x8 rs = *(const bf16x8*)((const __bf16*)p.m + P * 64 + co);
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (__bf16)(v[j] + p.bias[co + j] + (float)rs[j]);
            *(bf16x8*)((__bf16*)p.y + P * 64 + co) = o;
        }
}

// the generic kernels' fragment layout (pack_frag_kernel mode 0, bf16_gconv.hip) of rows [k0, k0 + kcount) of the input-channel axis of
// a Keras (kh,kw,cin_total,cout) kernel, padded with zeros to kpad x mpad:
//   out[((t*ksteps + ks)*mblocks + mb)*64 + lane][j] = W(m = mb*32 + (lane&31), k = ks*16 + 8*(lane>>5) + j, tap t)
__global__ void incep_pack_frag_kernel(const float* __restrict__ w, __bf16* __restrict__ out, int taps, int cin_total, int cout, int k0, int kcount,
                                       int kpad, int mpad) {
    const int ksteps = kpad >> 4, mblocks = mpad >> 5;
    const long total = (long)taps * kpad * mpad;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int j = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
        long q = idx >> 9;
        const int mb = (int)(q % mblocks); q /= mblocks;
        const int ks = (int)(q % ksteps);
        const int t = (int)(q / ksteps);
        const int m = mb * 32 + (lane & 31), k = ks * 16 + 8 * (lane >> 5) + j;
        const float v = m < cout && k < kcount ? w[((long)t * cin_total + k0 + k) * cout + m] : 0.f;
        out[idx] = (__bf16)v;
    }
}

// the epilogue vectors of a layer with c output channels, padded with zeros to cpad: the layer's bias and the inference-mode
// BatchNormalization + PReLU of its single consumer (bn_fold_kernel's arithmetic, norm.hip)
__global__ void incep_fold_kernel(const float* bias, const float* mmean, const float* mvar, const float* gamma, const float* beta, const float* alpha,
                                  int c, int cpad, float eps, float* scale, float* shift, float* alpha_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cpad) return;
    float sc = 0.f, sh = 0.f, al = 0.f;
    if (i < c) {
        const float b = bias ? bias[i] : 0.f;
        if (mmean) {
            sc = (gamma ? gamma[i] : 1.f) * rsqrtf(mvar[i] + eps);
            sh = (b - mmean[i]) * sc + (beta ? beta[i] : 0.f);
        } else {
            sc = 1.f;
            sh = b;
        }
        al = alpha ? alpha[i] : 0.f;
    }
    scale[i] = sc;
    shift[i] = sh;
    if (alpha_out) alpha_out[i] = al;
}

int pad32(int c) { return (c + 31) & ~31; }

}  // namespace

extern "C" {

int32_t vcg_incep_padded_channels(int32_t c) { return c > 0 ? pad32(c) : 0; }

size_t vcg_incep_frag_bf16_bytes(int32_t taps, int32_t cin, int32_t cout) {
    if (taps <= 0 || cin <= 0 || cout <= 0) return 0;
    return (size_t)taps * pad32(cin) * pad32(cout) * 2;
}

int vcg_pack_incep_frag_bf16(const float* w, int32_t taps, int32_t cin_total, int32_t cout, int32_t k0, int32_t kcount, void* out,
                             hipStream_t stream) {
    VCG_CHECK_PTR(w); VCG_CHECK_PTR(out);
    if (taps <= 0 || cin_total <= 0 || cout <= 0 || kcount <= 0 || k0 < 0 || k0 + kcount > cin_total) return VCG_E_SHAPE;
    if (taps > 25 || cout > 64 || kcount > 64) return VCG_E_UNSUPPORTED;
    const int kpad = pad32(kcount), mpad = pad32(cout);
    const long total = (long)taps * kpad * mpad;
    hipLaunchKernelGGL(incep_pack_frag_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, w, (__bf16*)out, taps, cin_total, cout, k0,
                       kcount, kpad, mpad);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

int vcg_incep_fold(const float* bias, const float* moving_mean, const float* moving_var, const float* gamma, const float* beta, const float* alpha,
                   int32_t c, float eps, float* scale, float* shift, float* alpha_out, hipStream_t stream) {
    VCG_CHECK_PTR(scale); VCG_CHECK_PTR(shift);
    if ((moving_mean == nullptr) != (moving_var == nullptr)) return VCG_E_NULL;
    if ((alpha == nullptr) != (alpha_out == nullptr)) return VCG_E_NULL;
    if (c <= 0) return VCG_E_SHAPE;
    if (c > 64) return VCG_E_UNSUPPORTED;
    hipLaunchKernelGGL(incep_fold_kernel, dim3(1), dim3(64), 0, stream, bias, moving_mean, moving_var, gamma, beta, alpha, c, pad32(c), eps, scale, shift,
                       alpha_out);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

int vcg_incep_head_bf16_fwd(const vcg_incep_head_desc* d, const void* m, const vcg_incep_head_path* paths, hipStream_t stream) {
    if (d == nullptr) return VCG_E_NULL;
    VCG_CHECK_PTR(m); VCG_CHECK_PTR(paths);
    if (d->n <= 0 || d->h <= 0 || d->w <= 0) return VCG_E_SHAPE;
    if (d->cin != 64 || d->npaths < 1 || d->npaths > IC_MAXPATHS) return VCG_E_UNSUPPORTED;
    const long pixels = (long)d->n * d->h * d->w;
    if (pixels * 128 > 0xFFFFFFE0l) return VCG_E_SHAPE;
    IhParams p{};
    p.m = m; p.pixels = pixels; p.npaths = d->npaths;
    for (int i = 0; i < d->npaths; ++i) {
        const vcg_incep_head_path& s = paths[i];
        if (d->cout[i] < 1) return VCG_E_SHAPE;
        if (d->cout[i] > 32) return VCG_E_UNSUPPORTED;
        VCG_CHECK_PTR(s.in_scale); VCG_CHECK_PTR(s.in_shift); VCG_CHECK_PTR(s.in_alpha); VCG_CHECK_PTR(s.wfrag);
        VCG_CHECK_PTR(s.out_scale); VCG_CHECK_PTR(s.out_shift); VCG_CHECK_PTR(s.y);
        p.p[i] = IhPath{s.in_scale, s.in_shift, s.in_alpha, s.wfrag, s.out_scale, s.out_shift, s.out_alpha, s.y};
    }
    hipLaunchKernelGGL(incep_head_bf16_kernel, dim3((unsigned)((pixels + 127) / 128)), dim3(256), 0, stream, p);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

int vcg_incep_join_bf16_fwd(const vcg_incep_join_desc* d, const void* const* z, const void* const* wfrag, const float* bias, const void* m, void* y,
                            hipStream_t stream) {
    if (d == nullptr) return VCG_E_NULL;
    VCG_CHECK_PTR(z); VCG_CHECK_PTR(wfrag); VCG_CHECK_PTR(bias); VCG_CHECK_PTR(m); VCG_CHECK_PTR(y);
    if (d->n <= 0 || d->h <= 0 || d->w <= 0) return VCG_E_SHAPE;
    if (d->cout != 64 || d->nsrc < 1 || d->nsrc > IC_MAXSRC) return VCG_E_UNSUPPORTED;
    const long pixels = (long)d->n * d->h * d->w;
    if (pixels * 128 > 0xFFFFFFE0l) return VCG_E_SHAPE;
    IjParams p{};
    p.nsrc = d->nsrc; p.bias = bias; p.m = m; p.y = y; p.pixels = pixels;
    for (int i = 0; i < d->nsrc; ++i) {
        if (d->cin[i] < 1) return VCG_E_SHAPE;
        if (d->cin[i] > 64) return VCG_E_UNSUPPORTED;
        VCG_CHECK_PTR(z[i]); VCG_CHECK_PTR(wfrag[i]);
        if (z[i] == y) return VCG_E_UNSUPPORTED;
        p.z[i] = z[i]; p.wf[i] = wfrag[i]; p.zc[i] = pad32(d->cin[i]);
    }
    hipLaunchKernelGGL(incep_join_bf16_kernel, dim3((unsigned)((pixels + 127) / 128)), dim3(256), 0, stream, p);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

}  // extern "C"
