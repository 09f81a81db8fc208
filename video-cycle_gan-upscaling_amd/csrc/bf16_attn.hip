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
    const __bf16* yin;       // bf16 NHWC [n][s h][s w][cout]: the LeakyReLU's output
    __bf16* y;               // the sum, same shape; yin itself in the in-place form
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
            const long yo = (((long)img * oh + oy) * ow + ox) * cout + c8 * 8;
            const bf16x8 yv = *(const bf16x8*)(p.yin + yo);
            bf16x8 ov;
#pragma unroll
            for (int j = 0; j < 8; ++j) ov[j] = (__bf16)((float)yv[j] + acc[j]);          // fp32 sum, rounded once
            *(bf16x8*)(p.y + yo) = ov;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The backward of add_input (model.py:94-97 differentiated) in one pass over the gradient dY at the block's output:
//     dz           = y_act > 0 ? dY : bf16(dY slope)         the gradient in front of the stage's LeakyReLU (vcg_lrelu_bwd_bf16's rule)
//     dbias_convt  = sum of the stored dz                     the stage's Conv2DTranspose bias
//     dbias_to_add = sum of dY
//     dw[ty][tx][co][ci] = sum a[ci][iy][ix] dY[s iy + ty][s ix + tx][co],   a = atanh(0.99999 x) as the forward evaluates it
// dY is read once, y_act once, dz written once: the kernel is bound by those three streams (3..12 FMAs per loaded element, no MFMA).
// The forward's index arithmetic read backwards: output pixel o = s i + t, t = o % s, feeds tap t of input pixel i = o / s and -- where
// t == 0 -- tap s of input pixel i - 1; an output index s h or s w does not exist, which is the row / column 'same' crops behind.
// A thread owns one unit = (output phase (ty, tx), 8 channels) and walks input pixels of its workgroup's TIH x TIW tiles; the IB_NT / units
// teams of a workgroup share a tile's pixels.  It keeps 8 x 3 sums for each of the up to four taps its phase feeds -- slot 0: (ty, tx);
// slot 1: (s, tx), ty == 0; slot 2: (ty, s), tx == 0; slot 3: (s, s) -- and the two bias sums of its 8 channels in registers for the whole
// launch: a slot the phase does not feed multiplies by a zero.  The sums go to the workspace as [workgroup][team][value][unit] records
// (consecutive threads, consecutive words) and are added up in a fixed order by a second kernel.
constexpr int IB_NT = 256, IB_MAX_GRID = 512;     // 112 accumulators per thread: two workgroups per CU
constexpr int IB_VALS = 4 * 24 + 16;              // per unit: [slot][channel][ci], sum dY [8], sum dz [8]
constexpr int IB_PF = 4;                          // pixels whose loads are in flight together

struct IcbParams {
    const float* x;          // fp32 NCHW [n][3][h][w]
    const __bf16* dy;        // bf16 NHWC [n][s h][s w][cout]
    const __bf16* yact;      // the LeakyReLU's output, same shape
    __bf16* dz;              // same shape
    float* ws;               // [gridDim.x * teams][IB_VALS][units]
    int n, h, w_, cout, tiles_x, tiles_y, total, units, teams;
    float scale, slope;
};

template <int S>
__global__ __launch_bounds__(IB_NT, 2) void input_convt_add_bf16_bwd_kernel(IcbParams p) {
    __shared__ __attribute__((aligned(16))) float lt[NHALO * 4];          // atanh of the halo pixels, RGB0: as the forward
    const int tid = threadIdx.x, cout = p.cout, tpp = cout >> 3;
    const int team = tid / p.units, unit = tid - team * p.units;
    const bool live = team < p.teams;
    const int c8 = unit % tpp, ph = unit / tpp, tx = ph % S, ty = ph / S;
    const bool up = ty == 0, left = tx == 0;
    float acc[4][24], sy[8], sz[8];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < 24; ++i) acc[k][i] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) sy[j] = sz[j] = 0.f;

    const long plane = (long)p.h * p.w_;
    const int oh = p.h * S, ow = p.w_ * S;
    for (int tile = blockIdx.x; tile < p.total; tile += gridDim.x) {
        const int txi = tile % p.tiles_x, t2 = tile / p.tiles_x, tyi = t2 % p.tiles_y, img = t2 / p.tiles_y;
        const int iy0 = tyi * TIH, ix0 = txi * TIW;
        __syncthreads();                                      // the previous tile's readers are done
        if (tid < NHALO * 3) {
            const int pix = tid / 3, ci = tid - 3 * pix, r = pix / (TIW + 1), c = pix - r * (TIW + 1);
            const int iy = iy0 - 1 + r, ix = ix0 - 1 + c;
            float t = 0.f;
            if (iy >= 0 && iy < p.h && ix >= 0 && ix < p.w_)
                t = (float)atanh((double)p.scale * (double)p.x[((long)img * 3 + ci) * plane + (long)iy * p.w_ + ix]);
            lt[pix * 4 + ci] = t;
            if (ci == 0) lt[pix * 4 + 3] = 0.f;
        }
        __syncthreads();
        if (!live) continue;

        for (int p0 = team; p0 < TIH * TIW; p0 += IB_PF * p.teams) {
            bf16x8 g[IB_PF], mk[IB_PF];
            long off[IB_PF];
            bool ok[IB_PF];
            int hp[IB_PF];
#pragma unroll
            for (int k = 0; k < IB_PF; ++k) {
                const int pix = p0 + k * p.teams, r = pix / TIW, c = pix - r * TIW, iy = iy0 + r, ix = ix0 + c;
                ok[k] = pix < TIH * TIW && iy < p.h && ix < p.w_;
                hp[k] = ok[k] ? (r + 1) * (TIW + 1) + c + 1 : TIW + 2;
                off[k] = ok[k] ? (((long)img * oh + iy * S + ty) * ow + ix * S + tx) * cout + c8 * 8 : (long)c8 * 8;
                g[k] = *(const bf16x8*)(p.dy + off[k]);
                mk[k] = *(const bf16x8*)(p.yact + off[k]);
            }
#pragma unroll
            for (int k = 0; k < IB_PF; ++k) {
                if (!ok[k]) continue;
                bf16x8 zv;
                float gf[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    gf[j] = (float)g[k][j];
                    zv[j] = (float)mk[k][j] > 0.f ? g[k][j] : (__bf16)(gf[j] * p.slope);
                    sy[j] += gf[j];
                    sz[j] += (float)zv[j];                    // the value as stored
                }
                *(bf16x8*)(p.dz + off[k]) = zv;
                // input pixel (iy, ix) and its neighbours above / to the left (zeros outside the image)
                f32x4 a[4];
                a[0] = *(const f32x4*)(lt + hp[k] * 4);
                a[1] = *(const f32x4*)(lt + (hp[k] - (TIW + 1)) * 4);
                a[2] = *(const f32x4*)(lt + (hp[k] - 1) * 4);
                a[3] = *(const f32x4*)(lt + (hp[k] - (TIW + 1) - 1) * 4);
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) {
                    a[1][ci] = up ? a[1][ci] : 0.f;
                    a[2][ci] = left ? a[2][ci] : 0.f;
                    a[3][ci] = up && left ? a[3][ci] : 0.f;
                }
#pragma unroll
                for (int sl = 0; sl < 4; ++sl)
#pragma unroll
                    for (int j = 0; j < 8; ++j)
#pragma unroll
                        for (int ci = 0; ci < 3; ++ci) acc[sl][j * 3 + ci] = fmaf(a[sl][ci], gf[j], acc[sl][j * 3 + ci]);
            }
        }
    }
    if (!live) return;
    float* out = p.ws + (long)(blockIdx.x * p.teams + team) * IB_VALS * p.units + unit;
#pragma unroll
    for (int sl = 0; sl < 4; ++sl)
#pragma unroll
        for (int i = 0; i < 24; ++i) out[(long)(sl * 24 + i) * p.units] = acc[sl][i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        out[(long)(96 + j) * p.units] = sy[j];
        out[(long)(104 + j) * p.units] = sz[j];
    }
}

// the records added up in a fixed order: one thread per (value, unit) of the weight gradient, per (value, 8-channel group) of the bias sums
// (those also run over the s x s phases); the decoded position is only used for the single store
__global__ __launch_bounds__(256) void input_convt_add_bf16_bwd_reduce_kernel(const float* __restrict__ ws, int nrec, int units, int cout, int s,
                                                                              float* __restrict__ dw, float* __restrict__ db_add,
                                                                              float* __restrict__ db_convt) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= IB_VALS * units) return;
    const int e = idx / units, unit = idx - e * units, tpp = cout >> 3, c8 = unit % tpp, ph = unit / tpp, tx = ph % s, ty = ph / s;
    const long stride = (long)IB_VALS * units;
    auto sum = [&](const float* src) {
        float t = 0.f;
#pragma unroll 8
        for (int r = 0; r < nrec; ++r) t += src[r * stride];
        return t;
    };
    if (e < 96) {
        const int sl = e / 24, rem = e - 24 * sl, j = rem / 3, ci = rem - 3 * j;
        if (((sl & 1) && ty) || ((sl & 2) && tx)) return;          // a slot this phase does not feed
        const int ky = (sl & 1) ? s : ty, kx = (sl & 2) ? s : tx;
        dw[((long)(ky * (s + 1) + kx) * cout + c8 * 8 + j) * 3 + ci] = sum(ws + (long)e * units + unit);
        return;
    }
    float* dst = e < 104 ? db_add : db_convt;
    if (ph != 0 || dst == nullptr) return;
    float t = 0.f;
    for (int q = 0; q < s * s; ++q) t += sum(ws + (long)e * units + q * tpp + c8);
    dst[c8 * 8 + ((e - 96) & 7)] = t;
}

// units, teams and workgroups of the backward for a served shape
static void icb_geometry(const vcg_conv_desc* d, int& units, int& teams, int& grid, long& total) {
    units = d->stride * d->stride * (d->cout >> 3);
    teams = IB_NT / units;
    if (teams > TIH * TIW) teams = TIH * TIW;
    total = (long)d->n * ceil_div(d->w, TIW) * ceil_div(d->h, TIH);
    grid = (int)(total < IB_MAX_GRID ? total : IB_MAX_GRID);
}

static int ica_check(const vcg_conv_desc* d) {
    const int s = d->stride;
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || s <= 0 || d->oh != d->h * s || d->ow != d->w * s) return VCG_E_SHAPE;
    if ((s != 2 && s != 4) || d->cin != 3 || d->kh != s + 1 || d->kw != s + 1 || d->pad_top != 0 || d->pad_left != 0 || d->cout <= 0 ||
        d->cout % 8 != 0)
        return VCG_E_UNSUPPORTED;
    return VCG_OK;
}

}  // namespace

extern "C" {

int vcg_input_convt_add_bf16_to(const vcg_conv_desc* d, const void* x, const void* w_hwoi, const void* bias, const void* y_in, void* y_out,
                                hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(x);
    VCG_CHECK_PTR(w_hwoi);
    VCG_CHECK_PTR(y_in);
    VCG_CHECK_PTR(y_out);
    if (int e = ica_check(d)) return e;
    const int s = d->stride;
    const size_t lds = ((size_t)(s + 1) * (s + 1) * 3 * d->cout + d->cout + NHALO * 4) * sizeof(float);
    if (lds > 64 * 1024) return VCG_E_UNSUPPORTED;
    IcaParams p;
    p.x = (const float*)x;
    p.w = (const float*)w_hwoi;
    p.bias = (const float*)bias;
    p.yin = (const __bf16*)y_in;
    p.y = (__bf16*)y_out;
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

int vcg_input_convt_add_bf16(const vcg_conv_desc* d, const void* x, const void* w_hwoi, const void* bias, void* y, hipStream_t stream) {
    return vcg_input_convt_add_bf16_to(d, x, w_hwoi, bias, y, y, stream);
}

size_t vcg_input_convt_add_bf16_bwd_ws_bytes(const vcg_conv_desc* d) {
    if (d == nullptr || ica_check(d) != VCG_OK || d->stride * d->stride * (d->cout >> 3) > IB_NT) return 0;
    int units, teams, grid;
    long total;
    icb_geometry(d, units, teams, grid, total);
    if (total > 0x7FFFFFFFl) return 0;
    return (size_t)grid * teams * IB_VALS * units * sizeof(float);
}

int vcg_input_convt_add_bf16_bwd(const vcg_conv_desc* d, const void* x, const void* dY, const void* y_act, float slope, void* dz, float* dw_hwoi,
                                 float* dbias_to_add, float* dbias_convt, void* ws, size_t ws_bytes, hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(x);
    VCG_CHECK_PTR(dY);
    VCG_CHECK_PTR(y_act);
    VCG_CHECK_PTR(dz);
    VCG_CHECK_PTR(dw_hwoi);
    VCG_CHECK_PTR(ws);
    if (int e = ica_check(d)) return e;
    if (dz == dY || dz == y_act) return VCG_E_UNSUPPORTED;        // dY is also the gradient of to_add_input; y_act's sign is the mask
    const size_t need = vcg_input_convt_add_bf16_bwd_ws_bytes(d);
    if (need == 0) return VCG_E_UNSUPPORTED;                      // more than IB_NT units (s = 4: cout > 128), or too many tiles
    if (ws_bytes < need) return VCG_E_WORKSPACE;
    IcbParams p;
    int grid;
    long total;
    icb_geometry(d, p.units, p.teams, grid, total);
    p.x = (const float*)x;
    p.dy = (const __bf16*)dY;
    p.yact = (const __bf16*)y_act;
    p.dz = (__bf16*)dz;
    p.ws = (float*)ws;
    p.n = d->n; p.h = d->h; p.w_ = d->w; p.cout = d->cout;
    p.tiles_x = ceil_div(d->w, TIW);
    p.tiles_y = ceil_div(d->h, TIH);
    p.total = (int)total;
    p.scale = 0.99999f;
    p.slope = slope;
    if (d->stride == 2) input_convt_add_bf16_bwd_kernel<2><<<grid, IB_NT, 0, stream>>>(p);
    else input_convt_add_bf16_bwd_kernel<4><<<grid, IB_NT, 0, stream>>>(p);
    VCG_LAUNCH_CHECK();
    input_convt_add_bf16_bwd_reduce_kernel<<<ceil_div(IB_VALS * p.units, 256), 256, 0, stream>>>((const float*)ws, grid * p.teams, p.units, p.cout,
                                                                                                  d->stride, dw_hwoi, dbias_to_add, dbias_convt);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

}  // extern "C"
