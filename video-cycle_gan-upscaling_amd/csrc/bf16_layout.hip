// bf16-storage path: layout conversion, weight packing and the PReLU backward passes at the entry of the bf16 trunk
// (bf16_tiles.hpp: why the bf16 path is NHWC)
#include "vcg_common.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// layout / packing helpers
// ---------------------------------------------------------------------------------------------------------------
__global__ void pack_kernel_bf16(const float* __restrict__ w, __bf16* __restrict__ out, int taps, int a, int b,
                                 int transpose, int flip) {
    // out[tap'][i][j] (j contiguous) = transpose ? w[tap][j][i] : w[tap][i][j];  tap' = flip ? taps-1-tap : tap
    const long total = (long)taps * a * b;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int j = (int)(idx % b);
        const int i = (int)((idx / b) % a);
        const int t = (int)(idx / ((long)a * b));
        const int ts = flip ? taps - 1 - t : t;
        const float v = transpose ? w[((long)ts * b + j) * a + i] : w[((long)ts * a + i) * b + j];
        out[idx] = (__bf16)v;
    }
}

// Every 3x3 64 -> 64 kernel of a model in ONE launch (the trunk re-derives 2 x 19 bf16 copies after each optimizer step: 38 launches of
// 4.7 us otherwise): blockIdx.y = layer, out[layer][0] = forward pack [tap][co][ci], out[layer][1] = data-gradient pack [8 - tap][ci][co].
constexpr int PACK_BATCH_MAX = 48;
struct PackBatch {
    const float* w[PACK_BATCH_MAX];
};
__global__ void pack3x3_c64_batch_kernel(PackBatch pb, __bf16* __restrict__ out) {
    const float* w = pb.w[blockIdx.y];
    __bf16* o = out + (long)blockIdx.y * 2 * 9 * 64 * 64;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < 2 * 9 * 64 * 64; idx += gridDim.x * blockDim.x) {
        const int which = idx / (9 * 64 * 64), r = idx - which * 9 * 64 * 64;
        const int j = r & 63, i = (r >> 6) & 63, t = r >> 12;
        // Keras (3,3,in,out): w[tap][ci][co].  forward: out[t][co=i][ci=j] (transpose); data gradient: out[t][ci=i][co=j] of tap 8 - t (flip)
        const float v = which == 0 ? w[(t * 64 + j) * 64 + i] : w[((8 - t) * 64 + i) * 64 + j];
        o[idx] = (__bf16)v;
    }
}

__global__ void f32_nchw_to_bf16_nhwc_kernel(const float* __restrict__ x, __bf16* __restrict__ y, int n, int c, int hw) {
    // one block per (n, 64-pixel segment): coalesced reads along pixels, coalesced writes along channels
    __shared__ float tile[64][65];
    const int p0 = blockIdx.x * 64, img = blockIdx.y;
    for (int c0 = 0; c0 < c; c0 += 64) {
        for (int e = threadIdx.x; e < 64 * 64; e += blockDim.x) {
            const int cc = e >> 6, pp = e & 63;
            float v = 0.f;
            if (c0 + cc < c && p0 + pp < hw) v = x[((long)img * c + c0 + cc) * hw + p0 + pp];
            tile[cc][pp] = v;
        }
        __syncthreads();
        if ((c & 7) == 0) {
            // 16-byte stores: a thread packs 8 consecutive channels of one pixel (8 lanes = one pixel's 128 bytes)
            for (int e = threadIdx.x; e < 64 * 8; e += blockDim.x) {
                const int pp = e >> 3, ch = (e & 7) * 8;
                if (c0 + ch < c && p0 + pp < hw) {
                    bf16x8 v;
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = (__bf16)tile[ch + j][pp];
                    *(bf16x8*)(y + ((long)img * hw + p0 + pp) * c + c0 + ch) = v;
                }
            }
        } else {
            for (int e = threadIdx.x; e < 64 * 64; e += blockDim.x) {
                const int pp = e >> 6, cc = e & 63;
                if (c0 + cc < c && p0 + pp < hw) y[((long)img * hw + p0 + pp) * c + c0 + cc] = (__bf16)tile[cc][pp];
            }
        }
        __syncthreads();
    }
}

__global__ void bf16_nhwc_to_f32_nchw_kernel(const __bf16* __restrict__ x, float* __restrict__ y, int n, int c, int hw) {
    __shared__ float tile[64][65];
    const int p0 = blockIdx.x * 64, img = blockIdx.y;
    for (int c0 = 0; c0 < c; c0 += 64) {
        if ((c & 7) == 0) {
            // 16-byte loads: a thread takes 8 consecutive channels of one pixel
            for (int e = threadIdx.x; e < 64 * 8; e += blockDim.x) {
                const int pp = e >> 3, ch = (e & 7) * 8;
                bf16x8 v;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.f;
                if (c0 + ch < c && p0 + pp < hw) v = *(const bf16x8*)(x + ((long)img * hw + p0 + pp) * c + c0 + ch);
#pragma unroll
                for (int j = 0; j < 8; ++j) tile[ch + j][pp] = (float)v[j];
            }
        } else {
            for (int e = threadIdx.x; e < 64 * 64; e += blockDim.x) {
                const int pp = e >> 6, cc = e & 63;
                float v = 0.f;
                if (c0 + cc < c && p0 + pp < hw) v = (float)x[((long)img * hw + p0 + pp) * c + c0 + cc];
                tile[cc][pp] = v;
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < 64 * 64; e += blockDim.x) {
            const int cc = e >> 6, pp = e & 63;
            if (c0 + cc < c && p0 + pp < hw) y[((long)img * c + c0 + cc) * hw + p0 + pp] = tile[cc][pp];
        }
        __syncthreads();
    }
}

// PReLU backward at the entry of the bf16 trunk (initial/prelu, model.py:276): the two gradients that meet at its output -- the trunk's and
// the long skip's (model.py:285), both bf16 NHWC -- are added, multiplied by the activation's derivative (sign of the stored pre-activation
// z) and written as the fp32 NCHW tensor the 3-channel convolution's weight-gradient kernel reads; the slope gradient sum(d * z, z < 0)
// leaves as one record of c floats per workgroup (summed in a fixed order by sum_records_kernel).  c % 8 == 0, c <= 64 * gridDim-free loop.
__global__ __launch_bounds__(256) void prelu_bwd_bf16_to_f32_nchw_kernel(const __bf16* __restrict__ d1, const __bf16* __restrict__ d2,
                                                                         const __bf16* __restrict__ z, const float* __restrict__ alpha,
                                                                         float* __restrict__ dz, float* __restrict__ rec, int c, int hw, int tiles) {
    __shared__ float tile[64][65];
    __shared__ float red[32][64];
    const int img = blockIdx.y, tid = threadIdx.x;
    const int ch = (tid & 7) * 8;                       // this thread's channel octet inside a 64-channel chunk (the same in both passes below)
    for (int c0 = 0; c0 < c; c0 += 64) {
        float da[8], al[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            da[j] = 0.f;
            al[j] = c0 + ch + j < c ? alpha[c0 + ch + j] : 0.f;
        }
        for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
            const int p0 = t * 64;
#pragma unroll
            for (int e = tid; e < 64 * 8; e += 256) {
                const int pp = e >> 3;
                float g[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) g[j] = 0.f;
                if (c0 + ch < c && p0 + pp < hw) {
                    const long o = ((long)img * hw + p0 + pp) * c + c0 + ch;
                    const bf16x8 a = *(const bf16x8*)(d1 + o), zz = *(const bf16x8*)(z + o);
                    bf16x8 b;
#pragma unroll
                    for (int j = 0; j < 8; ++j) b[j] = (__bf16)0.f;
                    if (d2) b = *(const bf16x8*)(d2 + o);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float d = (float)a[j] + (float)b[j], zf = (float)zz[j];
                        g[j] = zf >= 0.f ? d : d * al[j];
                        da[j] += zf >= 0.f ? 0.f : d * zf;
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) tile[ch + j][pp] = g[j];
            }
            __syncthreads();
            for (int e = tid; e < 64 * 64; e += 256) {
                const int cc = e >> 6, pp = e & 63;
                if (c0 + cc < c && p0 + pp < hw) dz[((long)img * c + c0 + cc) * hw + p0 + pp] = tile[cc][pp];
            }
            __syncthreads();
        }
        // the 32 threads that share a channel octet add up in a fixed order
#pragma unroll
        for (int j = 0; j < 8; ++j) red[tid >> 3][ch + j] = da[j];
        __syncthreads();
        if (tid < 64 && c0 + tid < c) {
            float s = 0.f;
            for (int k = 0; k < 32; ++k) s += red[k][tid];
            rec[((long)img * gridDim.x + blockIdx.x) * c + c0 + tid] = s;
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" {

int vcg_pack_conv_kernel_bf16(const void* w, int32_t taps, int32_t a, int32_t b, int32_t transpose, int32_t flip, void* out,
                              hipStream_t stream) {
    VCG_CHECK_PTR(w);
    VCG_CHECK_PTR(out);
    if (taps <= 0 || a <= 0 || b <= 0) return VCG_E_SHAPE;
    const long total = (long)taps * a * b;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    pack_kernel_bf16<<<blocks, 256, 0, stream>>>((const float*)w, (__bf16*)out, taps, a, b, transpose, flip);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

int vcg_pack_conv3x3_c64_bf16_batch(const void* const* w_host_array, int32_t count, void* out, hipStream_t stream) {
    VCG_CHECK_PTR(w_host_array);
    VCG_CHECK_PTR(out);
    if (count <= 0 || count > PACK_BATCH_MAX) return VCG_E_SHAPE;
    PackBatch pb;
    for (int i = 0; i < count; ++i) {
        VCG_CHECK_PTR(w_host_array[i]);
        pb.w[i] = (const float*)w_host_array[i];
    }
    pack3x3_c64_batch_kernel<<<dim3(36, count), 256, 0, stream>>>(pb, (__bf16*)out);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

int vcg_f32_nchw_to_bf16_nhwc(const void* x, void* y, int32_t n, int32_t c, int32_t h, int32_t w, hipStream_t stream) {
    VCG_CHECK_PTR(x);
    VCG_CHECK_PTR(y);
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return VCG_E_SHAPE;
    dim3 grid(ceil_div(h * w, 64), n);
    f32_nchw_to_bf16_nhwc_kernel<<<grid, 256, 0, stream>>>((const float*)x, (__bf16*)y, n, c, h * w);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

int vcg_bf16_nhwc_to_f32_nchw(const void* x, void* y, int32_t n, int32_t c, int32_t h, int32_t w, hipStream_t stream) {
    VCG_CHECK_PTR(x);
    VCG_CHECK_PTR(y);
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return VCG_E_SHAPE;
    dim3 grid(ceil_div(h * w, 64), n);
    bf16_nhwc_to_f32_nchw_kernel<<<grid, 256, 0, stream>>>((const __bf16*)x, (float*)y, n, c, h * w);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

static int prelu_bwd_gridx(int hw) { const int t = ceil_div(hw, 64); return t < 128 ? t : 128; }

// the same with the result left in the bf16 NHWC layout (for the bf16 weight gradient of the 3-channel convolution, bf16_wgrad3.hip): no
// transposition, a thread owns 8 channels of a pixel; same record layout
__global__ __launch_bounds__(256) void prelu_bwd_bf16_nhwc_kernel(const __bf16* __restrict__ d1, const __bf16* __restrict__ d2, const __bf16* __restrict__ z,
                                                                  const float* __restrict__ alpha, __bf16* __restrict__ dz, float* __restrict__ rec, int c,
                                                                  int hw, int tiles) {
    __shared__ float red[32][64];
    const int img = blockIdx.y, tid = threadIdx.x;
    const int ch = (tid & 7) * 8;
    for (int c0 = 0; c0 < c; c0 += 64) {
        float da[8], al[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            da[j] = 0.f;
            al[j] = c0 + ch + j < c ? alpha[c0 + ch + j] : 0.f;
        }
        for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
            const int p0 = t * 64;
#pragma unroll
            for (int e = tid; e < 64 * 8; e += 256) {
                const int pp = e >> 3;
                if (c0 + ch < c && p0 + pp < hw) {
                    const long o = ((long)img * hw + p0 + pp) * c + c0 + ch;
                    const bf16x8 a = *(const bf16x8*)(d1 + o), zz = *(const bf16x8*)(z + o);
                    bf16x8 b;
#pragma unroll
                    for (int j = 0; j < 8; ++j) b[j] = (__bf16)0.f;
                    if (d2) b = *(const bf16x8*)(d2 + o);
                    bf16x8 g;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float d = (float)a[j] + (float)b[j], zf = (float)zz[j];
                        g[j] = (__bf16)(zf >= 0.f ? d : d * al[j]);
                        da[j] += zf >= 0.f ? 0.f : d * zf;
                    }
                    *(bf16x8*)(dz + o) = g;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) red[tid >> 3][ch + j] = da[j];
        __syncthreads();
        if (tid < 64 && c0 + tid < c) {
            float s = 0.f;
            for (int k = 0; k < 32; ++k) s += red[k][tid];
            rec[((long)img * gridDim.x + blockIdx.x) * c + c0 + tid] = s;
        }
        __syncthreads();
    }
}

int vcg_prelu_bwd_nhwc_bf16_records(int n, int hw) {
    if (n <= 0 || hw <= 0) return VCG_E_SHAPE;
    return n * prelu_bwd_gridx(hw);
}

int vcg_prelu_bwd_nhwc_bf16(const void* d1, const void* d2, const void* z, const float* prelu_alpha, int n, int c, int hw, float* dz_nchw,
                            float* records, hipStream_t stream) {
    VCG_CHECK_PTR(d1); VCG_CHECK_PTR(z); VCG_CHECK_PTR(prelu_alpha); VCG_CHECK_PTR(dz_nchw); VCG_CHECK_PTR(records);
    if (n <= 0 || c <= 0 || hw <= 0 || n > 65535) return VCG_E_SHAPE;
    if (c % 8) return VCG_E_UNSUPPORTED;
    prelu_bwd_bf16_to_f32_nchw_kernel<<<dim3(prelu_bwd_gridx(hw), n), 256, 0, stream>>>((const __bf16*)d1, (const __bf16*)d2, (const __bf16*)z, prelu_alpha,
                                                                                     dz_nchw, records, c, hw, ceil_div(hw, 64));
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

int vcg_prelu_bwd_nhwc_bf16_to_bf16(const void* d1, const void* d2, const void* z, const float* prelu_alpha, int n, int c, int hw, void* dz_nhwc,
                                    float* records, hipStream_t stream) {
    VCG_CHECK_PTR(d1); VCG_CHECK_PTR(z); VCG_CHECK_PTR(prelu_alpha); VCG_CHECK_PTR(dz_nhwc); VCG_CHECK_PTR(records);
    if (n <= 0 || c <= 0 || hw <= 0 || n > 65535) return VCG_E_SHAPE;
    if (c % 8) return VCG_E_UNSUPPORTED;
    prelu_bwd_bf16_nhwc_kernel<<<dim3(prelu_bwd_gridx(hw), n), 256, 0, stream>>>((const __bf16*)d1, (const __bf16*)d2, (const __bf16*)z, prelu_alpha,
                                                                              (__bf16*)dz_nhwc, records, c, hw, ceil_div(hw, 64));
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

}  // extern "C"
