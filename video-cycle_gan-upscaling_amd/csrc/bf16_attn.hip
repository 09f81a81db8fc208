// to_add_input of upsampling_block_attention (upscaling/upscaler/model.py:94-97) on the bf16 inference path:
//
//     y = bf16( y + bias[c] + Conv2DTranspose(cout, kernel s+1, strides s, 'same')(atanh(0.99999 x))[c] )
//
// in place on the bf16 NHWC output y [n][s h][s w][cout] of the stage's LeakyReLU; x is the fp32 NCHW frames [n][3][h][w].
//
// 'same' with kernel s+1 and strides s crops nothing in front ((k - s) / 2 = 0) and one row / column behind, so
//     out[o] = sum_i t[i] w[o - s i],   0 <= o - s i <= s:   i = o / s with tap o % s, and -- where o % s == 0 and i >= 1 -- i - 1 with tap s.
// An output pixel therefore receives at most 2 x 2 input pixels x 3 channels: the kernel is element-wise on y and bound by reading and
// writing it.  A workgroup walks output tiles of (s TIH) x (s TIW) pixels.  Per tile the atanh of the (TIH + 1) x (TIW + 1) x 3 input values
// that reach it is evaluated ONCE, in double exactly as atanh_scale_kernel does (elementwise.hip: at |x| = 1 the derivative is 5e4, the fp32
// path's parity rests on that evaluation), and kept as fp32 in LDS next to the 3 (s+1)^2 cout fp32 weights, which are loaded once per workgroup.
// A thread owns 8 channels of a pixel: one 16-byte load and one 16-byte store of y, consecutive threads on consecutive channels, then pixels.
#include "vcg_common.hpp"

namespace {

constexpr int TIH = 4, TIW = 8;                  // input pixels per tile
constexpr int NHALO = (TIH + 1) * (TIW + 1);     // with the row above and the column to the left
constexpr int ICA_NT = 256, ICA_MAX_GRID = 1024;

struct IcaParams {
    const float* x;          // fp32 NCHW [n][3][h][w]
    const float* w;          // Keras Conv2DTranspose kernel (s+1, s+1, cout, 3)
    const float* bias;       // [cout] or null
    __bf16* y;               // bf16 NHWC [n][s h][s w][cout], updated in place
    int n, h, w_, cout, tiles_x, tiles_y, total;
    float scale;             // 0.99999
};

template <int S>
__global__ __launch_bounds__(ICA_NT) void input_convt_add_bf16_kernel(IcaParams p) {
    constexpr int K = S + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* lw = (float*)smem;                                // [ky][kx][ci][cout]
    float* lb = lw + K * K * 3 * p.cout;                     // [cout]
    float* lt = lb + p.cout;                                 // [TIH + 1][TIW + 1][4]: atanh of the halo pixels, RGB0
    const int tid = threadIdx.x, cout = p.cout, tpp = cout >> 3;

    for (int i = tid; i < K * K * 3 * cout; i += ICA_NT) {
        const int co = i % cout, t3 = i / cout, ci = t3 % 3, tap = t3 / 3;
        lw[i] = p.w[(tap * cout + co) * 3 + ci];
    }
    for (int i = tid; i < cout; i += ICA_NT) lb[i] = p.bias ? p.bias[i] : 0.f;

    const long plane = (long)p.h * p.w_;
    const int oh = p.h * S, ow = p.w_ * S;
    for (int tile = blockIdx.x; tile < p.total; tile += gridDim.x) {
        const int txi = tile % p.tiles_x, t2 = tile / p.tiles_x, tyi = t2 % p.tiles_y, img = t2 / p.tiles_y;
        const int iy0 = tyi * TIH, ix0 = txi * TIW;
        __syncthreads();                                      // the previous tile's readers are done (and, first, the weights are in)
        if (tid < NHALO * 3) {
            const int pix = tid / 3, ci = tid - 3 * pix, r = pix / (TIW + 1), c = pix - r * (TIW + 1);
            const int iy = iy0 - 1 + r, ix = ix0 - 1 + c;
            float t = 0.f;
            if (iy >= 0 && iy < p.h && ix >= 0 && ix < p.w_)
                t = (float)atanh((double)p.scale * (double)p.x[((long)img * 3 + ci) * plane + (long)iy * p.w_ + ix]);
            lt[pix * 4 + ci] = t;
        }
        __syncthreads();

        const int items = S * TIH * S * TIW * tpp;
        for (int it = tid; it < items; it += ICA_NT) {
            const int c8 = it % tpp, px = it / tpp, lx = px % (S * TIW), ly = px / (S * TIW);
            const int oy = iy0 * S + ly, ox = ix0 * S + lx;
            if (oy >= oh || ox >= ow) continue;
            const int ry = ly / S + 1, ky = ly - (ly / S) * S, rx = lx / S + 1, kx = lx - (lx / S) * S;     // halo position of input pixel (o / s), tap o % s
            float acc[8];
            *(f32x4*)&acc[0] = *(const f32x4*)(lb + c8 * 8);
            *(f32x4*)&acc[4] = *(const f32x4*)(lb + c8 * 8 + 4);
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                if (dy && ky) continue;                                     // the second row contributes only where o % s == 0 (tap s)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    if (dx && kx) continue;
                    // a pixel above / left of the image holds zeros in the halo
                    const float* t = lt + ((ry - dy) * (TIW + 1) + rx - dx) * 4;
                    const float* wt = lw + (((dy ? S : ky) * K + (dx ? S : kx)) * 3) * cout + c8 * 8;
#pragma unroll
                    for (int ci = 0; ci < 3; ++ci) {
                        const float tv = t[ci];
                        const f32x4 w0 = *(const f32x4*)(wt + ci * cout), w1 = *(const f32x4*)(wt + ci * cout + 4);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            acc[j] = fmaf(tv, w0[j], acc[j]);
                            acc[4 + j] = fmaf(tv, w1[j], acc[4 + j]);
                        }
                    }
                }
            }
            __bf16* yp = p.y + (((long)img * oh + oy) * ow + ox) * cout + c8 * 8;
            const bf16x8 yv = *(const bf16x8*)yp;
            bf16x8 ov;
#pragma unroll
            for (int j = 0; j < 8; ++j) ov[j] = (__bf16)((float)yv[j] + acc[j]);          // fp32 sum, rounded once
            *(bf16x8*)yp = ov;
        }
    }
}

}  // namespace

extern "C" {

int vcg_input_convt_add_bf16(const vcg_conv_desc* d, const void* x, const void* w_hwoi, const void* bias, void* y, hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(x);
    VCG_CHECK_PTR(w_hwoi);
    VCG_CHECK_PTR(y);
    const int s = d->stride;
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || s <= 0 || d->oh != d->h * s || d->ow != d->w * s) return VCG_E_SHAPE;
    if ((s != 2 && s != 4) || d->cin != 3 || d->kh != s + 1 || d->kw != s + 1 || d->pad_top != 0 || d->pad_left != 0 || d->cout <= 0 ||
        d->cout % 8 != 0)
        return VCG_E_UNSUPPORTED;
    const size_t lds = ((size_t)(s + 1) * (s + 1) * 3 * d->cout + d->cout + NHALO * 4) * sizeof(float);
    if (lds > 64 * 1024) return VCG_E_UNSUPPORTED;
    IcaParams p;
    p.x = (const float*)x;
    p.w = (const float*)w_hwoi;
    p.bias = (const float*)bias;
    p.y = (__bf16*)y;
    p.n = d->n; p.h = d->h; p.w_ = d->w; p.cout = d->cout;
    p.tiles_x = ceil_div(d->w, TIW);
    p.tiles_y = ceil_div(d->h, TIH);
    const long total = (long)p.n * p.tiles_x * p.tiles_y;
    if (total > 0x7FFFFFFFl) return VCG_E_UNSUPPORTED;
    p.total = (int)total;
    p.scale = 0.99999f;
    const int grid = p.total < ICA_MAX_GRID ? p.total : ICA_MAX_GRID;
    if (s == 2) input_convt_add_bf16_kernel<2><<<grid, ICA_NT, lds, stream>>>(p);
    else input_convt_add_bf16_kernel<4><<<grid, ICA_NT, lds, stream>>>(p);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

}  // extern "C"
