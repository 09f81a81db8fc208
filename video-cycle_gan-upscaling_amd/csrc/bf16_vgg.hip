// The bandwidth kernels of the bf16 VGG19 perceptual loss (VGG_LOSS / VGG_MSE_LOSS / VGG_MAE_LOSS, upscaling/upscaler/model.py:101-157) on
// bf16 NHWC activations: 2x2 max pooling forward, its backward fused with the ReLU derivative of the convolution in front of the pool, and
// the feature loss (value + gradient in front of block5_conv4's ReLU).  The sixteen convolutions run on bf16_conv3x3_3ch.hip / bf16_gconv.hip.
//
// Every lane moves 8 channels (16 bytes) per access with the channel axis fastest, so a wave reads and writes whole pixels back to back.
// No LDS, no atomics: the loss sum goes wave shuffles -> one partial per wave in the workspace -> one wave adds them in a fixed order.
#include "vcg_common.hpp"

namespace {

constexpr int VG_THREADS = 256;
constexpr int FL_MAX_BLOCKS = 1024;           // the loss kernel's grid: 4 partials (one per wave) each

__device__ __forceinline__ float bf_f32(unsigned hi16) { return __uint_as_float(hi16); }          // a bf16 held in the high half of a word

// the first maximal element of a 2x2 window in row-major order (torch / TF), compared as values: v[] hold the four bf16 in the high half
__device__ __forceinline__ int first_max(const unsigned (&v)[4], unsigned& bits) {
    int arg = 0;
    bits = v[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (bf_f32(v[k]) > bf_f32(bits)) { bits = v[k]; arg = k; }
    return arg;
}

__device__ __forceinline__ unsigned word_of(const uint4& q, int j) { return j == 0 ? q.x : j == 1 ? q.y : j == 2 ? q.z : q.w; }
__device__ __forceinline__ void set_word(uint4& q, int j, unsigned v) {
    if (j == 0) q.x = v; else if (j == 1) q.y = v; else if (j == 2) q.z = v; else q.w = v;
}

// x [n][h][w][c] -> y [n][h/2][w/2][c]; one lane per output pixel and 8 channels
__global__ __launch_bounds__(VG_THREADS) void maxpool2x2_nhwc_bf16_fwd_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, size_t total,
                                                                               int h, int w, int c8) {
    const size_t i = (size_t)blockIdx.x * VG_THREADS + threadIdx.x;
    if (i >= total) return;
    const int oh = h >> 1, ow = w >> 1;
    const int cg = (int)(i % c8);
    const size_t px = i / c8;
    const int ox = (int)(px % ow), oy = (int)((px / ow) % oh);
    const size_t nn = px / ((size_t)ow * oh);
    const size_t row = (size_t)w * c8;
    const uint4* s = x + ((nn * h + 2 * oy) * (size_t)w + 2 * ox) * c8 + cg;
    const uint4 q[4] = {s[0], s[c8], s[row], s[row + c8]};
    uint4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned lo[4], hi[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned wd = word_of(q[k], j);
            lo[k] = wd << 16;
            hi[k] = wd & 0xffff0000u;
        }
        unsigned ml, mh;
        first_max(lo, ml);
        first_max(hi, mh);
        set_word(o, j, (ml >> 16) | mh);
    }
    y[i] = o;
}

// dz [n][h][w][c] from the pool's input a = relu(z) and the gradient dy [n][h/2][w/2][c] at its output: dy to the first maximal element of
// each window if that element is > 0, zero elsewhere.  One lane per window (complete or cut off by an odd h / w) and 8 channels: every
// element of dz is written exactly once.
__global__ __launch_bounds__(VG_THREADS) void maxpool2x2_relu_nhwc_bf16_bwd_kernel(const uint4* __restrict__ a, const uint4* __restrict__ dy,
                                                                                    uint4* __restrict__ dz, size_t total, int h, int w, int c8) {
    const size_t i = (size_t)blockIdx.x * VG_THREADS + threadIdx.x;
    if (i >= total) return;
    const int oh = h >> 1, ow = w >> 1, wh = (h + 1) >> 1, ww = (w + 1) >> 1;
    const int cg = (int)(i % c8);
    const size_t win = i / c8;
    const int wx = (int)(win % ww), wy = (int)((win / ww) % wh);
    const size_t nn = win / ((size_t)ww * wh);
    const size_t row = (size_t)w * c8;
    const size_t base = ((nn * h + 2 * wy) * (size_t)w + 2 * wx) * c8 + cg;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    if (wy >= oh || wx >= ow) {                 // a window cut off by the last row / column: its pixels take part in no pooling
        dz[base] = zero;
        if (2 * wx + 1 < w) dz[base + c8] = zero;
        if (2 * wy + 1 < h) {
            dz[base + row] = zero;
            if (2 * wx + 1 < w) dz[base + row + c8] = zero;
        }
        return;
    }
    const uint4 q[4] = {a[base], a[base + c8], a[base + row], a[base + row + c8]};
    const uint4 g = dy[((nn * oh + wy) * (size_t)ow + wx) * c8 + cg];
    uint4 o[4] = {zero, zero, zero, zero};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned lo[4], hi[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned wd = word_of(q[k], j);
            lo[k] = wd << 16;
            hi[k] = wd & 0xffff0000u;
        }
        unsigned ml, mh;
        const int al = first_max(lo, ml), ah = first_max(hi, mh);
        const unsigned gw = word_of(g, j);
        const unsigned gl = bf_f32(ml) > 0.f ? (gw & 0xffffu) : 0u;
        const unsigned gh = bf_f32(mh) > 0.f ? (gw & 0xffff0000u) : 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) set_word(o[k], j, (k == al ? gl : 0u) | (k == ah ? gh : 0u));
    }
    dz[base] = o[0];
    dz[base + c8] = o[1];
    dz[base + row] = o[2];
    dz[base + row + c8] = o[3];
}

// one feature: the loss term into acc, the bf16 gradient in front of block5_conv4's ReLU as the return value (low 16 bits)
__device__ __forceinline__ unsigned loss_elem(float t, float p, int kind, float gs, float& acc) {
    const float d = p - t;
    float g;
    if (kind == VCG_LOSS_MSE) {
        acc += d * d;
        g = 2.f * d * gs;
    } else {
        acc += fabsf(d);
        g = d > 0.f ? gs : (d < 0.f ? -gs : 0.f);
    }
    if (!(p > 0.f)) g = 0.f;
    return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)g);
}

__global__ __launch_bounds__(VG_THREADS) void feature_loss_bf16_kernel(const unsigned short* __restrict__ ft, const unsigned short* __restrict__ fp,
                                                                       size_t count, int kind, float gs, float* __restrict__ part,
                                                                       unsigned short* __restrict__ dz) {
    const size_t nvec = count >> 3;
    const uint4* t4 = (const uint4*)ft;
    const uint4* p4 = (const uint4*)fp;
    uint4* d4 = (uint4*)dz;
    float acc = 0.f;
    for (size_t i = (size_t)blockIdx.x * VG_THREADS + threadIdx.x; i < nvec; i += (size_t)gridDim.x * VG_THREADS) {
        const uint4 tv = t4[i], pv = p4[i];
        uint4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned tw = word_of(tv, j), pw = word_of(pv, j);
            const unsigned lo = loss_elem(bf_f32(tw << 16), bf_f32(pw << 16), kind, gs, acc);
            const unsigned hi = loss_elem(bf_f32(tw & 0xffff0000u), bf_f32(pw & 0xffff0000u), kind, gs, acc);
            set_word(o, j, lo | (hi << 16));
        }
        d4[i] = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)(count & 7)) {          // the last count % 8 features
        const size_t i = (nvec << 3) + threadIdx.x;
        dz[i] = (unsigned short)loss_elem(bf_f32((unsigned)ft[i] << 16), bf_f32((unsigned)fp[i] << 16), kind, gs, acc);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[blockIdx.x * (VG_THREADS / 64) + (threadIdx.x >> 6)] = acc;
}

// one wave: lane l adds partials l, l + 64, ... in double, then a butterfly -- the same order on every run
__global__ __launch_bounds__(64) void feature_loss_final_kernel(const float* __restrict__ part, int nparts, double inv_count, float* __restrict__ out) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) s += (double)part[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) out[0] = (float)(s * inv_count);
}

int fl_blocks(size_t count) {
    const size_t nb = ((count >> 3) + VG_THREADS - 1) / VG_THREADS;
    return nb < 1 ? 1 : (nb > FL_MAX_BLOCKS ? FL_MAX_BLOCKS : (int)nb);
}

int pool_check(const void* a, const void* b, const void* c, int n, int h, int w, int ch) {
    if (a == nullptr || b == nullptr || c == nullptr) return VCG_E_NULL;
    if (n <= 0 || ch <= 0 || h < 2 || w < 2) return VCG_E_SHAPE;
    if (ch % 8 || (((size_t)a | (size_t)b | (size_t)c) & 15)) return VCG_E_UNSUPPORTED;
    return VCG_OK;
}

}  // namespace

extern "C" {

int vcg_maxpool2x2_nhwc_bf16_fwd(const void* x, void* y, int32_t n, int32_t h, int32_t w, int32_t c, hipStream_t stream) {
    if (int e = pool_check(x, y, x, n, h, w, c)) return e;
    const int c8 = c / 8;
    const size_t total = (size_t)n * (h / 2) * (w / 2) * c8;
    const size_t blocks = (total + VG_THREADS - 1) / VG_THREADS;
    if (blocks > 0x7fffffffull) return VCG_E_SHAPE;
    hipLaunchKernelGGL(maxpool2x2_nhwc_bf16_fwd_kernel, dim3((unsigned)blocks), dim3(VG_THREADS), 0, stream, (const uint4*)x, (uint4*)y, total, h, w, c8);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

int vcg_maxpool2x2_relu_nhwc_bf16_bwd(const void* y_prepool, const void* dy, void* dz, int32_t n, int32_t h, int32_t w, int32_t c,
                                      hipStream_t stream) {
    if (int e = pool_check(y_prepool, dy, dz, n, h, w, c)) return e;
    const int c8 = c / 8;
    const size_t total = (size_t)n * ((h + 1) / 2) * ((w + 1) / 2) * c8;
    const size_t blocks = (total + VG_THREADS - 1) / VG_THREADS;
    if (blocks > 0x7fffffffull) return VCG_E_SHAPE;
    hipLaunchKernelGGL(maxpool2x2_relu_nhwc_bf16_bwd_kernel, dim3((unsigned)blocks), dim3(VG_THREADS), 0, stream, (const uint4*)y_prepool,
                       (const uint4*)dy, (uint4*)dz, total, h, w, c8);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

size_t vcg_feature_loss_bf16_ws_bytes(size_t count) {
    return count == 0 ? 0 : (size_t)fl_blocks(count) * (VG_THREADS / 64) * sizeof(float);
}

int vcg_feature_loss_bf16(const void* f_true, const void* f_pred, size_t count, int32_t kind, float grad_scale, float* loss_out, void* dz_pred,
                          void* ws, size_t ws_bytes, hipStream_t stream) {
    VCG_CHECK_PTR(f_true); VCG_CHECK_PTR(f_pred); VCG_CHECK_PTR(loss_out); VCG_CHECK_PTR(dz_pred); VCG_CHECK_PTR(ws);
    if (count == 0) return VCG_E_SHAPE;
    if (kind != VCG_LOSS_MSE && kind != VCG_LOSS_MAE) return VCG_E_UNSUPPORTED;
    if ((((size_t)f_true | (size_t)f_pred | (size_t)dz_pred) & 15) || ((size_t)ws & 3)) return VCG_E_UNSUPPORTED;
    if (ws_bytes < vcg_feature_loss_bf16_ws_bytes(count)) return VCG_E_WORKSPACE;
    const int nb = fl_blocks(count);
    hipLaunchKernelGGL(feature_loss_bf16_kernel, dim3(nb), dim3(VG_THREADS), 0, stream, (const unsigned short*)f_true, (const unsigned short*)f_pred,
                       count, kind, (float)((double)grad_scale / (double)count), (float*)ws, (unsigned short*)dz_pred);
    VCG_LAUNCH_CHECK();
    hipLaunchKernelGGL(feature_loss_final_kernel, dim3(1), dim3(64), 0, stream, (const float*)ws, nb * (VG_THREADS / 64), 1.0 / (double)count, loss_out);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

}  // extern "C"
