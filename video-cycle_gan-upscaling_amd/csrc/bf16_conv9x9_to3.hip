// bf16 9x9 final convolution, 256 -> 3 channels (+ tanh): kernel, weight packing and C entry points.
#include "bf16_tiles.hpp"
#include "vcg_stamps.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// 9x9 stride-1 'same' convolution, 256 -> 3 channels (+bias, tanh): the generator's final/conv (model.py:290-291)
// ---------------------------------------------------------------------------------------------------------------
// Three output channels would waste 29 of the MFMA's 32 rows, so the rows carry (ky, co) instead:
//   row 4*ky+co (ky < 8)  and  row 4*co+3 (ky = 8);      k = (kx, ci);      columns = 32 consecutive x.
// One MFMA pass over ONE input row yi then yields, for every ky, that row's contribution to output row yi+4-ky.
// A wave marches down the image and carries the partial sums of the 9 output rows in flight IN THE ACCUMULATOR:
// before the next input row the accumulator is shifted by one ky-group (4 rows = half a register group: a
// v_permlane32_swap + select per register) and handed to the MFMA as its C operand; the group that falls off the end
// (ky = 7) lands in the spare rows 3,7,11, where the ky = 8 products complete it.  After the pass those three rows
// hold the finished output row yi-4 -- no atomics, no partial tensors, every input row is read from HBM once.
//   * the 256 input channels are split over the 4 waves of a workgroup (64 each): the 9x4 weight fragments of a
//     wave stay in 144 VGPRs; the four partial output rows meet in LDS once per row (768 B per wave);
//   * the wave's 72-pixel x 64-channel slice of the input row goes HBM -> LDS by global_load_lds (no VGPRs), double
//     buffered, XOR-swizzled on the global side so that the shifted ds_read_b128 of all 9 kx are conflict-free;
//   * work item = (image, 64-column strip, segment of 32..128 output rows); 2 workgroups per CU.
constexpr int F_PIX = 72;                    // 64 output columns + 4 + 4
constexpr int F_ROWB = F_PIX * 128;          // one wave's slice of one input row in LDS (9216 B)
// LDS of a workgroup of NW waves: NW * 2 * F_ROWB (row slices, double buffered) + 2 * NW * 3 * 64 * 4 (partial output rows)
constexpr int F9_MAX_GRID = 512;             // workgroups of one launch: two per CU
constexpr int F_NFRAG = 4 * 9 * 4 * 64;      // 16-byte weight fragments; the packed buffer holds 4 more (zeros)

struct F9Params {
    const unsigned char* x;      // bf16 NHWC [n][h][w][256]
    const uint4* wfrag;          // packed [4 chunks][9 kx][4 s][64 lanes] x 16 B, followed by 64 zero bytes
    const float* bias;           // [3] or null
    float* y;                    // fp32 NCHW [n][3][h][w]
    int n, h, w_, strips, segs, sh, total;      // sh: output rows per work item (8 halo rows are recomputed per item)
    int tanh_act;
};
// the window forms (OUT != F9_FULL): output rows [row0, row0 + rows) of x's images are computed and stored as rows [y_row0, y_row0 + rows)
// of images of y_h rows.  The new fields follow F9Params': the whole-image kernels keep their kernarg block, offsets and size
struct F9WinParams : F9Params {
    int row0, rows, y_row0, y_h;
};
// what a launch stores: the whole image as fp32 NCHW (vcg_conv9x9_to3_bf16_fwd), or a window of rows as fp32 NCHW / uint8 NHWC frames
// (vcg_conv9x9_to3_bf16_fwd_window)
constexpr int F9_FULL = 0, F9_WIN_F32 = 1, F9_WIN_U8 = 2;

// data.py:253-256, the expression of nchw_to_u8_kernel (elementwise.hip): uint8(around((a + 1) * 127.5)), round-half-even, clamped
__device__ __forceinline__ unsigned char f9_to_u8(float v) {
    return (unsigned char)fminf(fmaxf(rintf((v + 1.f) * 127.5f), 0.f), 255.f);
}

// Diagnostic build only (-DVCG_STAMPS, scripts/micro/stamps.py): s_memtime brackets around the five segments of an input row, summed
// per wave and written to a buffer of their own; no stamp executes in the shipped library.
VCG_STAMP_SUMS(f9, 512 * 4 * 8);

// tanh from one v_exp_f32 and one v_rcp_f32 (tanhf's libm expansion was ~100 instructions per output value on the three waves that
// finish a row while the fourth idles): 1 - 2 / (exp(2|x|) + 1), odd; below 2^-6 the cubic, where the quotient form would cancel.
// Absolute error < 2e-7, far below the bf16 operands' own rounding.
__device__ __forceinline__ float fast_tanh(float x) {
    const float a = fabsf(x);
    const float t = 1.f - 2.f * __frcp_rn(__expf(2.f * a) + 1.f);
    const float small = a * (1.f - a * a * (1.f / 3.f));
    return copysignf(a < 0.015625f ? small : t, x);
}

// window forms: output row yo of the input image is row y_row0 + (yo - row0) of an image of y_h rows
template <int OUT>
__device__ __forceinline__ void f9_store_win(const F9WinParams& p, int img, int yo, int x, int co, float v) {
    const int yr = p.y_row0 + (yo - p.row0);
    if constexpr (OUT == F9_WIN_U8) ((unsigned char*)p.y)[((long)(img * p.y_h + yr) * p.w_ + x) * 3 + co] = f9_to_u8(v);
    else p.y[((long)(img * 3 + co) * p.y_h + yr) * p.w_ + x] = v;
}

// BUF: the row slices are fetched through the image's buffer descriptor (pixels outside the image read as zero by the range check) with two
// lane constants; the pointer form (BUF = false: images too large for a descriptor) keeps nine 64-bit lane addresses, which at this kernel's
// 256-register budget are SPILLED -- hipcc then waits vmcnt(0) in front of every reload, i.e. for every earlier piece of the row: the nine
// pieces went out one HBM round trip after the other, 8.0 k of the 15.4 k cycles of a row (profiles/r03_f9_stamps.txt).
// NW: waves per workgroup = input channels / 64 (the channel split): 4 for the 256-channel final/conv of make_upscaler_orig, 2 for the
// 128-channel one of make_upscaler_attention (model.py:326).  A wave keeps its 64 channels, its 144 weight registers and its row slice
// either way; a pixel is NW x 128 bytes, the workgroup NW x 64 threads and NW x 18 KiB of row buffers (so twice as many fit a CU), and
// the NW partial rows meet in LDS as before.  NW = 1 (head/conv of make_generator_cyclegan on 64 channels; descriptor form only): a
// workgroup is one wave with 18 KiB of row buffers and two 768-byte partial rows, so eight fit a CU's LDS (2 waves per SIMD); the single
// partial row still goes through LDS, where the wave's own lanes re-read it as 3 x 64 outputs -- the barrier has nobody else to wait
// for, the lgkmcnt(0) in front of it is what orders the wave's stores before its loads, and a slot is rewritten two rows later.
// OUT: F9_FULL keeps the whole-image form's code exactly.  The window forms segment [row0, row0 + rows) instead of [0, h) -- the DMA of
// rows y0-4 .. y1+4 is the same, a row outside [0, h) still reads as zero -- and place the rows in an image of y_h rows.  F9_WIN_U8: the
// row's 64 pixels are 192 consecutive bytes of the NHWC frame; thread t of the 192 finishes BYTE t (co = t % 3, col = t / 3, the
// same four-term sum in the same order), so each of the three waves issues one byte store per lane to 64 consecutive addresses.  A row's
// base (row * w + x0) * 3 is not dword-aligned for general w: byte stores need no alignment case.
// P: the kernarg struct, F9Params for F9_FULL (its kernarg block is the one it always had) and F9WinParams for the window forms.
template <bool BUF, int NW = 4, int OUT = F9_FULL, class P = F9Params>
__global__ __launch_bounds__(64 * NW, 2) void conv9x9_c256to3_bf16_kernel(P p) {
    constexpr int PB = NW * 128;                                      // bytes per pixel
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long f0 = 0, f1 = 0, f2 = 0, f3 = 0, f4 = 0, f5 = 0, f6 = 0, fs_shift = 0, fs_wait = 0, fs_dma = 0, fs_mfma = 0, fs_bar = 0, fs_out = 0, f_rows = 0;
    (void)f6, (void)fs_shift, (void)f0, (void)f1, (void)f2, (void)f3, (void)f4, (void)f5, (void)fs_wait, (void)fs_dma, (void)fs_mfma, (void)fs_bar, (void)fs_out, (void)f_rows;
#ifdef VCG_STAMPS
    const unsigned long long k_c0 = __builtin_amdgcn_s_memtime(), k_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int c = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave = input-channel chunk
    unsigned char* rowbuf = smem + c * 2 * F_ROWB;
    float* part = (float*)(smem + NW * 2 * F_ROWB);                   // [2][NW][3][64]

    // weights: 36 fragments of 16 B per lane
    bf16x8 wf[9][4];
#pragma unroll
    for (int kx = 0; kx < 9; ++kx)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint4 v = p.wfrag[((c * 9 + kx) * 4 + s) * 64 + lane];
            wf[kx][s] = __builtin_bit_cast(bf16x8, v);
        }
    // B-fragment addresses: pixel (r+kx) of the slice, chunk (2s+h) ^ f(pixel);  addr = T[kx] ^ (s << 5)
    int T[9];
#pragma unroll
    for (int kx = 0; kx < 9; ++kx) {
        const int pos = r + kx;
        T[kx] = (pos * 128) | ((((pos >> 1) & 7) ^ hh) << 4);
    }
    // DMA slots of this lane: slot = k*64 + lane -> pixel = slot >> 3, stored chunk = slot & 7 holds channel chunk
    // (slot & 7) ^ f(pixel)
    // (recomputed per row from three lane constants: 18 more live VGPRs would spill)
    const int l3 = lane >> 3, l4 = lane >> 4, l7 = lane & 7;
    float bias = 0.f, bias3[3] = {0.f, 0.f, 0.f};
    if constexpr (NW == 4 && OUT == F9_WIN_U8) bias = (p.bias && tid < 192) ? p.bias[tid % 3] : 0.f;
    else if constexpr (NW == 4) bias = (p.bias && tid < 192) ? p.bias[tid >> 6] : 0.f;
    else if (p.bias) bias3[0] = p.bias[0], bias3[1] = p.bias[1], bias3[2] = p.bias[2];
    (void)bias, (void)bias3;
    const unsigned char* zeros = (const unsigned char*)(p.wfrag + NW * (F_NFRAG / 4));      // padding pixels are fetched from here
    // BUF: byte offset of this lane's slot of piece k relative to the piece's first pixel: pixel l3, source chunk of parity k & 1
    unsigned lc[2];
#pragma unroll
    for (int par = 0; par < 2; ++par) lc[par] = (unsigned)(l3 * PB + (c * 8 + (l7 ^ ((4 * par + l4) & 7))) * 16);
    const long img_bytes = (long)p.h * p.w_ * PB;

    for (int item = blockIdx.x; item < p.total; item += gridDim.x) {
        const int seg = item % p.segs, i2 = item / p.segs, strip = i2 % p.strips, img = i2 / p.strips;
        const int x0 = strip * 64, y0 = [&] { if constexpr (OUT == F9_FULL) return seg * p.sh; else return p.row0 + seg * p.sh; }(),
                  y1 = min(y0 + p.sh, [&] { if constexpr (OUT == F9_FULL) return p.h; else return p.row0 + p.rows; }());
        const vcg_rsrc rs = make_rsrc(p.x + img * img_bytes, (unsigned long)img_bytes);

        auto dma = [&](int yi, int buf) {
            if (BUF) {
                // offset = (row, first pixel of the strip's halo) + piece + lane constant, in 32-bit wrap-around arithmetic: a row above the
                // image lands just below 4 GiB, a row below it just past the image -- both outside the descriptor (host guard)
                const unsigned row_off = (unsigned)(yi * p.w_ + x0 - 4) * (unsigned)PB;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const int gx = x0 - 4 + k * 8 + l3;
                    unsigned off = row_off + (unsigned)(k * 8 * PB) + lc[k & 1];
                    asm volatile("" : "+v"(off));                    // a select, not a branch around the arithmetic
                    off = (unsigned)gx < (unsigned)p.w_ ? off : VCG_OOB;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (void __attribute__((address_space(3)))*)(rowbuf + buf * F_ROWB + k * 1024), 16, off, 0, 0, 0);
                }
                return;
            }
            const bool rowok = (unsigned)yi < (unsigned)p.h;
            const unsigned char* rowp = p.x + ((long)(img * p.h + (rowok ? yi : 0)) * p.w_) * PB;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int gx = x0 - 4 + k * 8 + l3;
                const bool ok = rowok && (unsigned)gx < (unsigned)p.w_;
                const int dsrc = (c * 8 + (l7 ^ ((4 * k + l4) & 7))) * 16;
                const unsigned char* src = ok ? rowp + (long)gx * PB + dsrc : zeros;
                __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src,
                                                 (void __attribute__((address_space(3)))*)(rowbuf + buf * F_ROWB + k * 1024), 16, 0, 0);
            }
        };

        f32x16 acc[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[tt][e] = 0.f;

        dma(y0 - 4, 0);
        for (int yi = y0 - 4; yi < y1 + 4; ++yi) {
            const int buf = (yi - (y0 - 4)) & 1;
            VCG_STAMP(f0);
            __builtin_amdgcn_s_waitcnt(0x0F70);              // vmcnt(0): this row's slice has landed in LDS
            asm volatile("" ::: "memory");
            VCG_STAMP(f1);
            if (yi + 1 < y1 + 4) dma(yi + 1, buf ^ 1);
            const unsigned char* xb = rowbuf + buf * F_ROWB;
            VCG_STAMP(f6);

            // shift the partial sums by one ky group and use them as the C operand.  Register by register, carrying the previous group's
            // upper halves: three temporaries instead of 32 (with all 16 swaps first the kernel spilled, and every scratch reload behind
            // an LDS-DMA costs a vmcnt(0))
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                float ph[3] = {0.f, 0.f, 0.f};                   // upper halves of the previous group (group 2jq-1 -> 2jq)
#pragma unroll
                for (int jq = 0; jq < 4; ++jq)
#pragma unroll
                    for (int sl = 0; sl < 3; ++sl) {
                        float a = acc[tt][4 * jq + sl], b = a;
                        swap32(a, b);                            // a = (lower, lower), b = (upper, upper)
                        acc[tt][4 * jq + sl] = hh ? a : ph[sl];  // group 2jq -> 2jq+1
                        ph[sl] = b;
                    }
                acc[tt][3] = hh ? ph[1] : ph[0];                 // rows 3 / 7  <- group 7, co 0 / 1
                acc[tt][7] = hh ? 0.f : ph[2];                   // row 11      <- group 7, co 2
                acc[tt][11] = 0.f;
                acc[tt][15] = 0.f;
            }

            VCG_STAMP(f2);
            bf16x8 fb[2][2];
            // an opaque zero in every fragment address: without it hipcc hoists all 36 (kx, s) addresses out of the row loop and keeps them
            // live in 36 registers -- this kernel has 9 to give (144 of its 256 hold the weights) and spilled the rest
            int opq = 0;
            asm volatile("" : "+v"(opq));
            auto frag = [&](auto ic) {
                constexpr int i = decltype(ic)::value, kx = i >> 2, s = i & 3, bq = i & 1;
                const unsigned char* a = xb + ((T[kx] + opq) ^ (s << 5));
                fb[bq][0] = *(const bf16x8*)(a);
                fb[bq][1] = *(const bf16x8*)(a + 32 * 128);
            };
            frag(std::integral_constant<int, 0>{});
            static_for<36>([&](auto ic) {
                constexpr int i = decltype(ic)::value, kx = i >> 2, s = i & 3, cur = i & 1;
                if constexpr (i + 1 < 36) frag(std::integral_constant<int, i + 1>{});
                __builtin_amdgcn_sched_barrier(0);
                acc[0] = mfma_bf16(wf[kx][s], fb[cur][0], acc[0]);
                acc[1] = mfma_bf16(wf[kx][s], fb[cur][1], acc[1]);
                __builtin_amdgcn_sched_barrier(0);
            });

            VCG_STAMP(f3);
            // finished output row yo = yi - 4: this wave's partial (its 64 input channels) -> LDS
            const int yo = yi - 4, slot = yo & 1;
            if (yo >= y0) {
                float* pp = part + ((slot * NW + c) * 3) * 64;
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    // rows 3 / 7 / 11 = co 0 (lower half) / 1 (upper half) / 2 (lower half): every lane stores register 3 to its co's row, the
                    // lower half register 7 as well (written as selects: hipcc turned the two-sided branch into a 16-way register select)
                    pp[hh * 64 + tt * 32 + r] = acc[tt][3];
                    if (hh == 0) pp[2 * 64 + tt * 32 + r] = acc[tt][7];
                }
            }
            // the partial sums are ordinary LDS stores: wait for them and meet.  NOT lds_barrier(): its fence makes hipcc drain vmcnt(0),
            // i.e. wait here for the NEXT row's slice, which nothing reads before the wait at the top of the next iteration
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            VCG_STAMP(f4);
            if constexpr (NW == 4) {
                if (yo >= y0 && tid < 192) {
                    int co_, col_;                                   // F9_WIN_U8: thread t finishes byte t of the row
                    if constexpr (OUT == F9_WIN_U8) { co_ = tid % 3; col_ = tid / 3; } else { co_ = tid >> 6; col_ = tid & 63; }
                    const int co = co_, col = col_;
                    const float* q = part + slot * 4 * 3 * 64 + co * 64 + col;
                    float v = ((q[0] + q[3 * 64]) + (q[2 * 3 * 64] + q[3 * 3 * 64])) + bias;
                    if (p.tanh_act) v = fast_tanh(v);
                    if constexpr (OUT == F9_FULL) {
                        if (x0 + col < p.w_) p.y[((long)(img * 3 + co) * p.h + yo) * p.w_ + x0 + col] = v;
                    } else if (x0 + col < p.w_) f9_store_win<OUT>(p, img, yo, x0 + col, co, v);
                }
            } else if (yo >= y0) {
                // 3 x 64 outputs of the row on NW x 64 threads
                for (int o = tid; o < 192; o += 64 * NW) {
                    int co_, col_;
                    if constexpr (OUT == F9_WIN_U8) { co_ = o % 3; col_ = o / 3; } else { co_ = o >> 6; col_ = o & 63; }
                    const int co = co_, col = col_;
                    const float* q = part + slot * NW * 3 * 64 + co * 64 + col;
                    float v = q[0];
#pragma unroll
                    for (int k = 1; k < NW; ++k) v += q[k * 3 * 64];
                    v += co == 0 ? bias3[0] : co == 1 ? bias3[1] : bias3[2];
                    if (p.tanh_act) v = fast_tanh(v);
                    if constexpr (OUT == F9_FULL) {
                        if (x0 + col < p.w_) p.y[((long)(img * 3 + co) * p.h + yo) * p.w_ + x0 + col] = v;
                    } else if (x0 + col < p.w_) f9_store_win<OUT>(p, img, yo, x0 + col, co, v);
                }
            }
            VCG_STAMP(f5);
            VCG_STAMP_ADD(fs_wait, f0, f1); VCG_STAMP_ADD(fs_dma, f1, f6); VCG_STAMP_ADD(fs_shift, f6, f2); VCG_STAMP_ADD(fs_mfma, f2, f3); VCG_STAMP_ADD(fs_bar, f3, f4); VCG_STAMP_ADD(fs_out, f4, f5);
            VCG_STAMP_ADD(f_rows, 0ull, 1ull);
        }
        lds_barrier();       // the next item's first partial slot / row buffers are free
    }
#ifdef VCG_STAMPS
    if (lane == 0 && blockIdx.x < 512) {
        unsigned long long* o = vcg_f9_stamp_sums + (blockIdx.x * 4 + c) * 8;
        o[0] = fs_wait, o[1] = fs_dma, o[2] = fs_mfma, o[3] = fs_bar, o[4] = fs_out, o[5] = f_rows;
        o[6] = __builtin_amdgcn_s_memtime() - k_c0, o[7] = fs_shift;
    }
#endif
}

__global__ void pack_final9x9_kernel(const float* __restrict__ w, uint4* __restrict__ out, int cin) {
    // w: Keras (9,9,cin,3) -> out[chunk][kx][s][lane] = 8 bf16: A[row = lane&31][k = 8*(lane>>5) + j] of k-step (kx, s)
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int nfrag = (cin >> 6) * (F_NFRAG / 4);
    if (idx >= nfrag + 4) return;
    if (idx >= nfrag) {
        out[idx] = make_uint4(0, 0, 0, 0);
        return;
    }
    const int lane = idx & 63, s = (idx >> 6) & 3, kx = (idx >> 8) % 9, c = idx / (9 * 256);
    const int row = lane & 31, h = lane >> 5, g = row >> 2, sl = row & 3;
    int ky = -1, co = 0;
    if (sl < 3) { ky = g; co = sl; }
    else if (g < 3) { ky = 8; co = g; }
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = c * 64 + 16 * s + 8 * h + j;
        v[j] = (__bf16)(ky >= 0 ? w[((ky * 9 + kx) * cin + ci) * 3 + co] : 0.f);
    }
    out[idx] = __builtin_bit_cast(uint4, v);
}

// c64: the entry points of head/conv on 64 channels (vcg_conv9x9_c64to3_bf16_*), which serve that channel count alone; the others keep
// answering VCG_E_UNSUPPORTED for it
int f9_check_desc(const vcg_conv_desc* d, bool c64 = false) {
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->oh != d->h || d->ow != d->w) return VCG_E_SHAPE;
    if ((c64 ? d->cin != 64 : d->cin != 256 && d->cin != 128) || d->cout != 3 || d->kh != 9 || d->kw != 9 || d->stride != 1 || d->pad_top != 4 ||
        d->pad_left != 4)
        return VCG_E_UNSUPPORTED;
    return VCG_OK;
}

// plan and launch of both entry points.  out = F9_FULL: the whole image (row0 = 0, rows = d->h); the window forms compute output rows
// [row0, row0 + rows) only and exist for the descriptor form alone
int f9_launch(const vcg_conv_desc* d, const void* x, const void* wfrag, const void* bias, int tanh_act, void* y, int out, int row0, int rows,
              int y_row0, int y_h, hipStream_t stream) {
    const int nw = d->cin / 64;
    const int max_grid = F9_MAX_GRID * 4 / nw;                    // half the threads and LDS per workgroup: twice the workgroups per CU
    // the descriptor form needs the image, four rows above and four below it inside 32-bit offsets
    const bool buf = ((long)d->h + 8) * d->w * (nw * 128) + 65536 <= 0xFFFFFFE0l;
    // (a caller bands the image so that this never happens; the 64-channel layer has the descriptor form alone)
    if ((out != F9_FULL || nw == 1) && !buf) return VCG_E_UNSUPPORTED;
    F9WinParams p;
    p.x = (const unsigned char*)x;
    p.wfrag = (const uint4*)wfrag;
    p.bias = (const float*)bias;
    p.y = (float*)y;
    p.n = d->n;
    p.h = d->h;
    p.w_ = d->w;
    p.strips = ceil_div(d->w, 64);
    p.row0 = row0, p.rows = rows, p.y_row0 = y_row0, p.y_h = y_h;
    // segments per column strip: the split that minimises the rows the busiest workgroup marches through -- rounds of items per
    // workgroup x (segment height + 8 recomputed halo rows).  (Round 2 halved the height until the items filled the grid twice: 25 % halo
    // rows at C3's shape, and at C4's 1080 items on 512 workgroups = a third round for 56 of them.)
    {
        long best = -1;
        const int colstrips = p.n * p.strips;
        for (int segs = 1; segs <= ceil_div(rows, 16); ++segs) {
            const int sh = ceil_div(rows, segs);
            if (ceil_div(rows, sh) != segs) continue;                             // (the same height reached with fewer segments)
            const long items = (long)colstrips * segs, rounds = (items + max_grid - 1) / max_grid, cost = rounds * (sh + 8);
            if (best < 0 || cost < best) { best = cost; p.sh = sh; p.segs = segs; }
        }
    }
    p.total = p.n * p.strips * p.segs;
    p.tanh_act = tanh_act;
    const int grid = p.total < max_grid ? p.total : max_grid;
#define VCG_F9_LAUNCH(KERNEL, NW, ARG) do {                                                                                \
        constexpr int lds = NW * 2 * F_ROWB + 2 * NW * 3 * 64 * 4;                                                         \
        if (int e = vcg_allow_dyn_lds((const void*)KERNEL, lds)) return e;                                                 \
        KERNEL<<<grid, 64 * NW, lds, stream>>>(ARG);                                                                        \
    } while (0)
    const F9Params& whole = p;
    if (nw == 1) {               // one wave per workgroup: 2048 workgroups of 19.5 KiB of LDS, eight per CU
        if (out == F9_WIN_F32) VCG_F9_LAUNCH((conv9x9_c256to3_bf16_kernel<true, 1, F9_WIN_F32, F9WinParams>), 1, p);
        else if (out == F9_WIN_U8) VCG_F9_LAUNCH((conv9x9_c256to3_bf16_kernel<true, 1, F9_WIN_U8, F9WinParams>), 1, p);
        else VCG_F9_LAUNCH((conv9x9_c256to3_bf16_kernel<true, 1>), 1, whole);
    } else if (out == F9_WIN_F32) {
        if (nw == 4) VCG_F9_LAUNCH((conv9x9_c256to3_bf16_kernel<true, 4, F9_WIN_F32, F9WinParams>), 4, p);
        else VCG_F9_LAUNCH((conv9x9_c256to3_bf16_kernel<true, 2, F9_WIN_F32, F9WinParams>), 2, p);
    } else if (out == F9_WIN_U8) {
        if (nw == 4) VCG_F9_LAUNCH((conv9x9_c256to3_bf16_kernel<true, 4, F9_WIN_U8, F9WinParams>), 4, p);
        else VCG_F9_LAUNCH((conv9x9_c256to3_bf16_kernel<true, 2, F9_WIN_U8, F9WinParams>), 2, p);
    } else if (nw == 4) {
        if (buf) VCG_F9_LAUNCH((conv9x9_c256to3_bf16_kernel<true, 4>), 4, whole); else VCG_F9_LAUNCH((conv9x9_c256to3_bf16_kernel<false, 4>), 4, whole);
    } else {
        if (buf) VCG_F9_LAUNCH((conv9x9_c256to3_bf16_kernel<true, 2>), 2, whole); else VCG_F9_LAUNCH((conv9x9_c256to3_bf16_kernel<false, 2>), 2, whole);
    }
#undef VCG_F9_LAUNCH
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

}  // namespace

extern "C" {

int vcg_pack_final9x9_bf16(const void* w, void* out, hipStream_t stream) {
    VCG_CHECK_PTR(w);
    VCG_CHECK_PTR(out);
    pack_final9x9_kernel<<<(F_NFRAG + 4 + 255) / 256, 256, 0, stream>>>((const float*)w, (uint4*)out, 256);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

size_t vcg_conv9x9_to3_bf16_wfrag_bytes(int32_t cin) {
    if (cin != 128 && cin != 256) return 0;
    return (size_t)((cin >> 6) * (F_NFRAG / 4) + 4) * 16;
}

int vcg_pack_conv9x9_to3_bf16(const void* w, int32_t cin, void* out, hipStream_t stream) {
    VCG_CHECK_PTR(w);
    VCG_CHECK_PTR(out);
    if (cin != 128 && cin != 256) return VCG_E_UNSUPPORTED;
    const int total = (cin >> 6) * (F_NFRAG / 4) + 4;
    pack_final9x9_kernel<<<(total + 255) / 256, 256, 0, stream>>>((const float*)w, (uint4*)out, cin);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

int vcg_conv9x9_to3_bf16_fwd(const vcg_conv_desc* d, const void* x, const void* wfrag, const void* bias, int32_t tanh_act, void* y,
                             hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(x);
    VCG_CHECK_PTR(wfrag);
    VCG_CHECK_PTR(y);
    if (int e = f9_check_desc(d)) return e;
    return f9_launch(d, x, wfrag, bias, tanh_act, y, F9_FULL, 0, d->h, 0, d->h, stream);
}

int vcg_conv9x9_to3_bf16_fwd_window(const vcg_conv_desc* d, const void* x, const void* wfrag, const void* bias, int32_t tanh_act,
                                    int32_t out_kind, void* y, int32_t row0, int32_t rows, int32_t y_row0, int32_t y_h, hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(x);
    VCG_CHECK_PTR(wfrag);
    VCG_CHECK_PTR(y);
    if (int e = f9_check_desc(d)) return e;
    if (rows <= 0 || row0 < 0 || (long)row0 + rows > d->h || y_row0 < 0 || (long)y_row0 + rows > y_h) return VCG_E_SHAPE;
    if (int e = f9_check_desc(d)) return e;
    if (out_kind != VCG_OUT_F32_NCHW && out_kind != VCG_OUT_U8_NHWC) return VCG_E_UNSUPPORTED;
    return f9_launch(d, x, wfrag, bias, tanh_act, y, out_kind == VCG_OUT_U8_NHWC ? F9_WIN_U8 : F9_WIN_F32, row0, rows, y_row0, y_h, stream);
}

// head/conv of make_generator_cyclegan: the same layer on 64 input channels, one wave per workgroup (NW = 1)
size_t vcg_conv9x9_c64to3_bf16_wfrag_bytes(void) { return (size_t)(F_NFRAG / 4 + 4) * 16; }

int vcg_pack_conv9x9_c64to3_bf16(const void* w, void* out, hipStream_t stream) {
    VCG_CHECK_PTR(w);
    VCG_CHECK_PTR(out);
    const int total = F_NFRAG / 4 + 4;
    pack_final9x9_kernel<<<(total + 255) / 256, 256, 0, stream>>>((const float*)w, (uint4*)out, 64);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

int vcg_conv9x9_c64to3_bf16_fwd(const vcg_conv_desc* d, const void* x, const void* wfrag, const void* bias, int32_t tanh_act, void* y,
                                hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(x);
    VCG_CHECK_PTR(wfrag);
    VCG_CHECK_PTR(y);
    if (int e = f9_check_desc(d, true)) return e;
    return f9_launch(d, x, wfrag, bias, tanh_act, y, F9_FULL, 0, d->h, 0, d->h, stream);
}

int vcg_conv9x9_c64to3_bf16_fwd_window(const vcg_conv_desc* d, const void* x, const void* wfrag, const void* bias, int32_t tanh_act,
                                       int32_t out_kind, void* y, int32_t row0, int32_t rows, int32_t y_row0, int32_t y_h, hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(x);
    VCG_CHECK_PTR(wfrag);
    VCG_CHECK_PTR(y);
    if (int e = f9_check_desc(d, true)) return e;
    if (rows <= 0 || row0 < 0 || (long)row0 + rows > d->h || y_row0 < 0 || (long)y_row0 + rows > y_h) return VCG_E_SHAPE;
    if (out_kind != VCG_OUT_F32_NCHW && out_kind != VCG_OUT_U8_NHWC) return VCG_E_UNSUPPORTED;
    return f9_launch(d, x, wfrag, bias, tanh_act, y, out_kind == VCG_OUT_U8_NHWC ? F9_WIN_U8 : F9_WIN_F32, row0, rows, y_row0, y_h, stream);
}

}  // extern "C"
