// Implicit-GEMM direct convolution on v_mfma_f32_32x32x2_f32 (exact fp32), NCHW.
//
// GEMM view:  M = output channels, N = output pixels (32 consecutive x of one row per MFMA tile),
//             K = (input channel, ky, kx).  The two k of one MFMA are two consecutive input
//             channels at the same tap, so every operand read is "lane base + immediate".
// Workgroup:  256 threads = 4 waves; tile = 64 output channels x (8 rows x 32 cols);
//             wave w owns rows 2w, 2w+1  ->  2x2 MFMA tiles, 64 accumulator VGPRs.
// Staging:    one LDS buffer holding CK input channels' halo tile + their weights; the next
//             chunk's global loads are issued into registers BEFORE the MFMA loop of the current
//             chunk and written to LDS after it (issue-early / write-late).
// Serves:     Conv2D forward (model.py:19,22,275,283,839-871), stride-1 Conv2D dgrad (flipped
//             taps, per-tap transposed kernel), Conv2DTranspose dgrad (stride-2 conv).
//
// Second kernel (conv_smallm): for <=32/KW output channels (final 9x9 256->3 conv, model.py:290;
// PatchGAN's 1-channel head; dgrad into 3-channel images) the M dimension of the MFMA carries
// (channel, kx) pairs and the kx shift-sum is done in the epilogue through LDS, so the matrix core
// runs at 27/32 row utilisation instead of 3/32.
#include "vcg_common.hpp"
#include <type_traits>

namespace {

struct ConvParams {
    const float* x;
    const float* w;        // [T][cin][cout]  (m contiguous)
    float* y;
    const float* bias;
    const float* prelu;
    const float* residual;
    int n, cin, h, w_, cout, oh, ow, pad_top, pad_left;
    int tiles_x, tiles_y, co_blocks;
    int act;
    float alpha;
    int flip;
    // small-M kernel only: weight element (mch, kc, tap) at w[tap*ws_t + mch*ws_m + kc*ws_k]
    int ws_t, ws_m, ws_k;
    float* stats;          // conv_fwd_kernel<..., STATS>: [n * tiles_y * tiles_x][2][cout] per-tile sums of the accumulators and of their squares
    // conv_fwd_kernel<..., AFFINE> only: per-channel scale / shift of an inference-mode normalisation between the bias and the activation
    const float* scale;
    const float* shift;
};

template <int KH, int KW, int S, int CK, int XT>
struct ConvCfg {
    static constexpr int ROWS = 8;
    static constexpr int IH = (ROWS - 1) * S + KH;
    static constexpr int IW = (32 * XT - 1) * S + KW;
    static constexpr int PLANE = IH * IW;
    static constexpr int T = KH * KW;
    static constexpr int IN_ELEMS = CK * PLANE;
    static constexpr int W_ELEMS = CK * T * 64;
    static constexpr int IN_PT = (IN_ELEMS + 255) / 256;
    static constexpr int W_PT = (W_ELEMS + 255) / 256;
    static constexpr size_t LDS_BYTES = (size_t)(IN_ELEMS + W_ELEMS) * sizeof(float);
};

// ---- shared epilogue: y = act(acc + bias) + residual for a 64-channel x (8 rows x 32*XT cols) tile ----------
// The (image, 64-channel block) of y -- and of the residual -- is one buffer descriptor and every address a 32-bit byte
// offset into it.  A lane keeps one offset per (row, x-tile) of its 2 x XT accumulator tiles: rows and columns past the
// ragged edge get VCG_OOB there, once per tile.  An element adds its channel's scalar multiple of the plane with a
// SATURATING add, so VCG_OOB stays out of range whatever is added (a wrapping add would bring it back into the block);
// channels past cout land behind num_records on their own.  The hardware drops what is out of range: one straight-line
// body, no exec-mask region.  The range check sees the VGPR offset only, which is why nothing sits in soffset.
// conv_block_fits() (host) keeps 64 planes below 4 GiB.
//
// AFFINE (an instantiation of its own: the launches without it run the kernels they always ran): v = acc + bias, rounded to fp32 as the stored
// output of the plain launch is; then v = fma(scale[c], v, shift[c]) and the activation in norm_act_fwd_kernel's form (PReLU as
// fma(alpha, min(v,0), max(v,0)): apply_act after contraction), so that the result has the bits of vcg_conv2d_fwd -> vcg_norm_act_fwd.
template <int XT, bool AFFINE = false>
__device__ __forceinline__ void conv_epilogue(const ConvParams& p, f32x16 (&acc)[2][2][XT], int n, int co0, int oy0, int ox0,
                                              int wv, int lane) {
    const int half = lane >> 5, l31 = lane & 31;
    const unsigned plane = (unsigned)(p.oh * p.ow), plane4 = 4u * plane, ow4 = 4u * (unsigned)p.ow;
    const int nch = p.cout - co0 < 64 ? p.cout - co0 : 64;
    const size_t blk = ((size_t)n * p.cout + co0) * plane;
    const size_t blk_bytes = (size_t)nch * plane * sizeof(float);
    const vcg_rsrc ry = make_rsrc(p.y + blk, blk_bytes);
    const vcg_rsrc rr = make_rsrc(p.residual ? p.residual + blk : nullptr, p.residual ? blk_bytes : 0);
    // none / LeakyReLU / PReLU share one straight-line form  v >= 0 ? v : v*slope  (slope 1 = identity);
    // tanh is only offered by the small-M kernel (the API rejects it here).  A missing bias / slope vector is an empty
    // descriptor: every load from it returns 0, like the loads of the channels past cout
    const bool is_prelu = p.act == VCG_ACT_PRELU;
    const vcg_rsrc rbias = make_rsrc(p.bias, p.bias ? (size_t)p.cout * sizeof(float) : 0);
    const vcg_rsrc rslope = make_rsrc(is_prelu ? p.prelu : nullptr, is_prelu ? (size_t)p.cout * sizeof(float) : 0);
    const float slope_u = (p.act == VCG_ACT_LRELU) ? p.alpha : 1.f;
    const unsigned chan4 = 4u * (unsigned)(co0 + 4 * half);
    const vcg_rsrc rscale = make_rsrc(AFFINE ? p.scale : nullptr, AFFINE ? (size_t)p.cout * sizeof(float) : 0);
    const vcg_rsrc rshift = make_rsrc(AFFINE ? p.shift : nullptr, AFFINE ? (size_t)p.cout * sizeof(float) : 0);

    const int oy = oy0 + wv * 2, ox = ox0 + l31;
    const unsigned base = (unsigned)(4 * half) * plane4 + (unsigned)oy * ow4 + 4u * (unsigned)ox;
    unsigned vo[2][XT];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int xt = 0; xt < XT; ++xt)
            vo[rt][xt] = (oy + rt < p.oh && ox + xt * 32 < p.ow) ? base + (unsigned)rt * ow4 + 128u * xt : VCG_OOB;

    // 16 elements = RG accumulator rows (channels) make a group; the residual of group g + 1 is requested before group g
    // is stored, so a group never waits for the stores in front of its own loads
    constexpr int RG = 8 / XT, NG = 32 / RG;
    auto emit = [&](auto res_tag, auto prelu_tag) {
        constexpr bool RES = decltype(res_tag)::value;
        constexpr bool PRELU_FMA = decltype(prelu_tag)::value;     // AFFINE with PReLU
        float rs[2][RG][2][XT];
        auto row_of = [](int g, int j) { const int q = g * RG + j, r = q & 15; return (q >> 4) * 32 + (r & 3) + 8 * (r >> 2); };
        auto load_res = [&](int g) {
#pragma unroll
            for (int j = 0; j < RG; ++j) {
                const unsigned srow = (unsigned)row_of(g, j) * plane4;
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int xt = 0; xt < XT; ++xt) rs[g & 1][j][rt][xt] = buf_load(rr, __builtin_elementwise_add_sat(vo[rt][xt], srow));
            }
        };
        if (RES) load_res(0);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            float bv[RG], al[RG], sc[RG], sh[RG];
#pragma unroll
            for (int j = 0; j < RG; ++j) {
                bv[j] = buf_load(rbias, chan4 + 4u * (unsigned)row_of(g, j));
                const float pa = buf_load(rslope, chan4 + 4u * (unsigned)row_of(g, j));
                al[j] = is_prelu ? pa : slope_u;
                if (AFFINE) {
                    sc[j] = buf_load(rscale, chan4 + 4u * (unsigned)row_of(g, j));
                    sh[j] = buf_load(rshift, chan4 + 4u * (unsigned)row_of(g, j));
                }
            }
            if (RES && g + 1 < NG) load_res(g + 1);
#pragma unroll
            for (int j = 0; j < RG; ++j) {
                const int q = g * RG + j;
                const unsigned srow = (unsigned)row_of(g, j) * plane4;
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
                    for (int xt = 0; xt < XT; ++xt) {
                        float v = acc[q >> 4][rt][xt][q & 15] + bv[j];
                        if (AFFINE) v = __builtin_fmaf(sc[j], v, sh[j]);
                        if (PRELU_FMA) v = __builtin_fmaf(al[j], fminf(v, 0.f), fmaxf(v, 0.f));
                        else v = v >= 0.f ? v : v * al[j];
                        if (RES) v += rs[g & 1][j][rt][xt];
                        buf_store(ry, __builtin_elementwise_add_sat(vo[rt][xt], srow), v);
                    }
                }
            }
        }
    };
    if constexpr (AFFINE) {
        if (is_prelu) {
            if (p.residual) emit(std::true_type{}, std::true_type{}); else emit(std::false_type{}, std::true_type{});
        } else {
            if (p.residual) emit(std::true_type{}, std::false_type{}); else emit(std::false_type{}, std::false_type{});
        }
    } else {
        if (p.residual) emit(std::true_type{}, std::false_type{}); else emit(std::false_type{}, std::false_type{});
    }
}

// STATS epilogue: for the BatchNormalization / instance norm behind the convolution (model.py:19-25, 840) the workgroup also leaves, per output
// channel, the sum of its tile's accumulators and of their squares -- the output minus the bias: a shift that keeps E[d^2] - E[d]^2 from
// cancelling -- as one record per tile; vcg_norm_finalize_partials_shifted sums the records in a fixed order.  The statistics pass over the
// output (one more read of the tensor, two more launches per normalisation) is gone.  A lane's 32 (channel) x 2 partial sums are
// reduce-scattered over the 32 lanes of its half-wave, the four waves (row pairs) meet in LDS.
template <int XT>
__device__ __forceinline__ void conv_stats_epilogue(const ConvParams& p, f32x16 (&acc)[2][2][XT], float* smem, int rec, int co0, int oy0, int ox0,
                                                    int wv, int lane, int tid) {
    const int half = lane >> 5, l31 = lane & 31;
    float sv[32], sq[32];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int xt = 0; xt < XT; ++xt) {
                    const bool ok = oy0 + wv * 2 + rt < p.oh && ox0 + l31 + xt * 32 < p.ow;
                    const float v = ok ? acc[mt][rt][xt][r] : 0.f;
                    a += v;
                    b = fmaf(v, v, b);
                }
            sv[mt * 16 + r] = a;
            sq[mt * 16 + r] = b;
        }
    const float ts = half_wave_reduce_scatter32(sv, l31), tq = half_wave_reduce_scatter32(sq, l31);
    // lane (l31, half) now holds value index l31 = (mt, r) summed over the half-wave's 32 columns: channel mt*32 + mfma_row(r)
    const int ch = (l31 >> 4) * 32 + (l31 & 3) + 8 * ((l31 & 15) >> 2) + 4 * half;
    __syncthreads();                                   // every wave is done with the operand tiles: the LDS is free
    smem[(0 * 4 + wv) * 64 + ch] = ts;
    smem[(1 * 4 + wv) * 64 + ch] = tq;
    __syncthreads();
    if (tid < 128) {
        const int st = tid >> 6, c = tid & 63;
        const float t = (smem[(st * 4 + 0) * 64 + c] + smem[(st * 4 + 1) * 64 + c]) + (smem[(st * 4 + 2) * 64 + c] + smem[(st * 4 + 3) * 64 + c]);
        if (co0 + c < p.cout) p.stats[((size_t)rec * 2 + st) * p.cout + co0 + c] = t;
    }
}

template <int KH, int KW, int S, int CK, int XT, bool STATS = false, bool AFFINE = false>
__global__ __launch_bounds__(256, (KH >= 9 ? 1 : 2)) void conv_fwd_kernel(const ConvParams p) {
    using C = ConvCfg<KH, KW, S, CK, XT>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_in = smem;               // [CK][IH][IW]
    float* s_w = smem + C::IN_ELEMS;  // [CK][T][64]

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    int b = blockIdx.x;
    const int cb = b % p.co_blocks; b /= p.co_blocks;
    const int tx = b % p.tiles_x;   b /= p.tiles_x;
    const int ty = b % p.tiles_y;   b /= p.tiles_y;
    const int n = b;
    const int ox0 = tx * 32 * XT, oy0 = ty * C::ROWS, co0 = cb * 64;
    const int gy0 = oy0 * S - p.pad_top, gx0 = ox0 * S - p.pad_left;
    const float* xn = p.x + (size_t)n * p.cin * p.h * p.w_;

    float rin[C::IN_PT], rw[C::W_PT];

    const int hw = p.h * p.w_;
    // weights: row q = (ci, tap) of the chunk is wave-uniform, the lane is the output channel.  Rows of channels past
    // cin alias the next tap's rows (finite values that meet zero inputs) or fall off the tensor's end (range check -> 0);
    // lanes past cout read the last valid column: their output rows are never stored
    const int wvu = __builtin_amdgcn_readfirstlane(wv);
    const unsigned wcol = 4u * (unsigned)(co0 + lane < p.cout ? co0 + lane : p.cout - 1);
    const size_t wbytes = (size_t)C::T * p.cin * p.cout * sizeof(float);

    auto in_rsrc = [&](int ci0) { return make_rsrc(xn + (size_t)ci0 * hw, (size_t)(p.cin - ci0) * hw * sizeof(float)); };
    auto load_w = [&](int ci0) {
        const vcg_rsrc rwt = make_rsrc(p.w + (size_t)ci0 * p.cout, wbytes - (size_t)ci0 * p.cout * sizeof(float));
#pragma unroll
        for (int i = 0; i < C::W_PT; ++i) {
            const int q = wvu + 4 * i;
            const int t = q % C::T, ci = q / C::T;
            const int tap = p.flip ? (C::T - 1 - t) : t;
            rw[i] = buf_load(rwt, 4u * (unsigned)((tap * p.cin + ci) * p.cout) + wcol);
        }
    };
    // the first chunk's weights need nothing of what follows: they are in flight while the input offsets are worked out
    load_w(0);
    __builtin_amdgcn_sched_barrier(0);                 // (the scheduler would otherwise sink them below the decode)

    // per-thread input BYTE offsets inside a chunk's [CK][h][w] block, computed once (VCG_OOB = zero padding); a chunk
    // only moves the descriptor's base (scalar), whose record count also cuts off the channels past cin: the
    // staging loop is one buffer_load per element, no per-element VALU and nothing that depends on the loaded data.
    // Element e = tid + 256 i is (channel, row, column) of the halo tile: decoded once for i = 0 and carried from e to
    // e + 256 with compare-and-subtract (256 = Q1 planes + QR rows + RC columns), the byte offset along with it (modulo
    // 2^32 while outside the map, exact inside).  Validity is a select on the offset.  Each element's load of the first
    // chunk leaves as soon as its offset is known.
    unsigned in_off[C::IN_PT];
    {
        constexpr int Q1 = 256 / C::PLANE, R1 = 256 % C::PLANE, QR = R1 / C::IW, RC = R1 % C::IW;
        const vcg_rsrc rx = in_rsrc(0);
        const unsigned w4 = 4u * (unsigned)p.w_, hw4 = 4u * (unsigned)hw;
        const unsigned step = (unsigned)Q1 * hw4 + (unsigned)QR * w4 + 4u * RC;
        const unsigned col_wrap = w4 - 4u * C::IW, row_wrap = hw4 - (unsigned)C::IH * w4;
        int ci = tid / C::PLANE, r = (tid % C::PLANE) / C::IW, c = (tid % C::PLANE) % C::IW;
        unsigned off = (unsigned)ci * hw4 + (unsigned)(gy0 + r) * w4 + 4u * (unsigned)(gx0 + c);
#pragma unroll
        for (int i = 0; i < C::IN_PT; ++i) {
            const bool in_tile = (i + 1) * 256 <= C::IN_ELEMS || ci < CK;
            const bool ok = in_tile && (unsigned)(gy0 + r) < (unsigned)p.h && (unsigned)(gx0 + c) < (unsigned)p.w_;
            in_off[i] = ok ? off : VCG_OOB;
            rin[i] = buf_load(rx, in_off[i]);
            __builtin_amdgcn_sched_barrier(0);         // keep the load here, not gathered behind the last offset
            c += RC;
            const bool cw = c >= C::IW;
            c -= cw ? C::IW : 0;
            r += QR + (cw ? 1 : 0);
            const bool rwr = r >= C::IH;
            r -= rwr ? C::IH : 0;
            ci += Q1 + (rwr ? 1 : 0);
            off += step + (cw ? col_wrap : 0u) + (rwr ? row_wrap : 0u);
        }
    }
    auto load_chunk = [&](int ci0) {
        const vcg_rsrc rx = in_rsrc(ci0);
#pragma unroll
        for (int i = 0; i < C::IN_PT; ++i) rin[i] = buf_load(rx, in_off[i]);
        load_w(ci0);
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < C::IN_PT; ++i) {
            const int e = tid + i * 256;
            if (e < C::IN_ELEMS) s_in[e] = rin[i];
        }
#pragma unroll
        for (int i = 0; i < C::W_PT; ++i) {
            const int e = tid + i * 256;
            if (e < C::W_ELEMS) s_w[e] = rw[i];
        }
    };

    f32x16 acc[2][2][XT];   // [co tile][row][x tile]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int x = 0; x < XT; ++x)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][x][r] = 0.f;

    const float* bbase = s_in + half * C::PLANE + (wv * 2 * S) * C::IW + l31 * S;
    const float* abase = s_w + half * C::T * 64 + l31;

    const int nchunks = (p.cin + CK - 1) / CK;
    for (int c = 0; c < nchunks; ++c) {
        __syncthreads();
        store_chunk();
        __syncthreads();
        if (c + 1 < nchunks) load_chunk((c + 1) * CK);   // in flight during this chunk's MFMAs
        // operand fragments are read one tap AHEAD of the MFMAs that use them (register double buffer, statically renamed
        // by the full unroll); sched_group_barrier pins the order "reads of tap t+1, then the 4*XT MFMAs of tap t", so a
        // wave's own LDS latency hides under its own MFMAs instead of relying on the SIMD's other wave
        constexpr int NTAP = (CK / 2) * C::T;
        auto rd = [&](int q, float (&a)[2], float (&b)[2][XT]) {
            const int cp = q / C::T, t = q % C::T, ky = t / KW, kx = t % KW;
            a[0] = abase[(cp * 2 * C::T + t) * 64];
            a[1] = abase[(cp * 2 * C::T + t) * 64 + 32];
#pragma unroll
            for (int xt = 0; xt < XT; ++xt) {
                b[0][xt] = bbase[cp * 2 * C::PLANE + ky * C::IW + kx + xt * 32 * S];
                b[1][xt] = bbase[cp * 2 * C::PLANE + (S + ky) * C::IW + kx + xt * 32 * S];
            }
        };
        float a_[2][2], b_[2][2][XT];
        rd(0, a_[0], b_[0]);
#pragma unroll
        for (int q = 0; q < NTAP; ++q) {
            const int cur = q & 1, nxt = cur ^ 1;
            if (q + 1 < NTAP) rd(q + 1, a_[nxt], b_[nxt]);
#pragma unroll
            for (int xt = 0; xt < XT; ++xt) {
                acc[0][0][xt] = mfma32(a_[cur][0], b_[cur][0][xt], acc[0][0][xt]);
                acc[0][1][xt] = mfma32(a_[cur][0], b_[cur][1][xt], acc[0][1][xt]);
                acc[1][0][xt] = mfma32(a_[cur][1], b_[cur][0][xt], acc[1][0][xt]);
                acc[1][1][xt] = mfma32(a_[cur][1], b_[cur][1][xt], acc[1][1][xt]);
            }
            if (q + 1 < NTAP) __builtin_amdgcn_sched_group_barrier(0x100, 1 + 2 * XT, 0);   // DS reads of the next tap first
            __builtin_amdgcn_sched_group_barrier(0x008, 4 * XT, 0);                          // then this tap's MFMAs
        }
    }

    conv_epilogue<XT, AFFINE>(p, acc, n, co0, oy0, ox0, wv, lane);
    if (STATS) conv_stats_epilogue<XT>(p, acc, smem, (n * p.tiles_y + ty) * p.tiles_x + tx, co0, oy0, ox0, wv, lane, tid);
}

// ------------------------------------------------------------------------------------------------
// <= 3 input channels (first 9x9 conv on RGB frames, model.py:275; data gradient of the final 9x9 conv, :290):
// the generic kernel pairs CHANNELS in the MFMA's k dimension and would pad 3 channels to 4 (25 % of the
// matrix work on zeros).  Here the whole (channel, ky, kx) range is one flat K axis staged once, and an MFMA
// takes two CONSECUTIVE k: the second half-wave reads one element further along the tap row, with the two
// row / channel wrap-arounds handled by two more per-lane base pointers chosen at compile time.
// A tile has few MFMAs (9x9: 488 a wave) against a 62.5 KB weight slab, so the kernel is persistent: a workgroup
// keeps its 64-channel block's weights in LDS and walks spatial tiles, the input tile double-buffered.
// ------------------------------------------------------------------------------------------------
template <int KH, int KW, int S>
struct C3Cfg {
    static constexpr int ROWS = 8;
    static constexpr int IH = (ROWS - 1) * S + KH;
    static constexpr int IW = 31 * S + KW;
    static constexpr int PLANE = IH * IW;
    static constexpr int T = KH * KW;
    static constexpr int KT = 3 * T;                       // flat K
    static constexpr int NP = (KT + 1) / 2;                // MFMA k-pairs
    static constexpr int IN_ELEMS = 3 * PLANE;
    static constexpr int W_ROWS = 2 * NP;                  // weight rows incl. one zero row when KT is odd
    static constexpr int W_ELEMS = W_ROWS * 64;
    static constexpr int IN_PT = (IN_ELEMS + 255) / 256;
    static constexpr int W_PT = W_ELEMS / 256;
    // one input buffer: the halo tile and four zero words.  When KT is odd the second half-wave's read behind the last k
    // lands on the first of them (its weight row is zero, but 0 * NaN is NaN: the word has to be finite)
    static constexpr int IN_BUF = IN_ELEMS + 4;
    static constexpr size_t LDS_BYTES = (size_t)(2 * IN_BUF + W_ELEMS) * sizeof(float);
    static_assert(IW < 256 && W_ELEMS % 256 == 0, "packed (row, column) of a halo element; whole weight rows per wave");
    static constexpr int off(int k) { return (k / T) * PLANE + ((k % T) / KW) * IW + (k % T) % KW; }
    static constexpr int D_ROW = IW - (KW - 1);                              // kx wraps to the next tap row
    static constexpr int D_CH = PLANE - (KH - 1) * IW - (KW - 1);            // last tap -> first tap of next channel
};

template <int KH, int KW, int S>
__global__ __launch_bounds__(256, 2) void conv_c3_kernel(const ConvParams p) {
    using C = C3Cfg<KH, KW, S>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_in = smem;                   // [2][IN_BUF]: halo tile [3][IH][IW] + zero words, double-buffered
    float* s_w = smem + 2 * C::IN_BUF;    // [W_ROWS][64]

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    // persistent: the workgroup keeps one 64-channel block, whose weights it stages once, and walks the spatial tiles
    // t, t + step, ... in (image, tile_y, tile_x) order; the coordinates are carried from tile to tile
    const int nblk = p.co_blocks, step = (int)gridDim.x / nblk;
    const int cb = (int)blockIdx.x % nblk, co0 = cb * 64;
    int t = (int)blockIdx.x / nblk;
    const int tiles = p.n * p.tiles_y * p.tiles_x;
    if (t >= tiles) return;
    int tx = t % p.tiles_x, ty = (t / p.tiles_x) % p.tiles_y, n = t / (p.tiles_x * p.tiles_y);
    const int dtx = step % p.tiles_x, dty = (step / p.tiles_x) % p.tiles_y, dn = step / (p.tiles_x * p.tiles_y);

    // ---- the thread's halo elements e = tid + 256 i: byte offset from the tile's first element and packed (row, column).
    // Decoded once per kernel where that costs at most 16 registers; the stride-2 tile (14 elements a thread) decodes
    // per tile, as every workgroup did before: held there, hipcc spills
    constexpr bool KEEP = C::IN_PT <= 8;
    const int hw = p.h * p.w_;
    const unsigned w4 = 4u * (unsigned)p.w_, hw4 = 4u * (unsigned)hw;
    const size_t img_bytes = (size_t)p.cin * hw * sizeof(float);
    auto decode = [&](int tid_, int i, unsigned& rel_, unsigned& rc_) {
        const int e = tid_ + i * 256;
        const int ci = e / C::PLANE, rem = e % C::PLANE;
        const int r = rem / C::IW, c = rem % C::IW;
        rel_ = (unsigned)ci * hw4 + (unsigned)r * w4 + 4u * (unsigned)c;
        rc_ = (unsigned)(r << 8 | c);
    };
    unsigned rel[KEEP ? C::IN_PT : 1], rc[KEEP ? C::IN_PT : 1];
    if constexpr (KEEP) {
#pragma unroll
        for (int i = 0; i < C::IN_PT; ++i) {
            decode(tid, i, rel[i], rc[i]);
            asm volatile("" : "+v"(rc[i]));            // one register: hipcc would carry row and column apart
        }
    }
    const bool last_live = tid + (C::IN_PT - 1) * 256 < C::IN_ELEMS;   // only the last element can lie past the tile
    // a tile's loads: one select per element, on the offset.  Padding and the ragged edge get VCG_OOB and read 0; a
    // channel past cin lies behind the image's records on its own (conv_block_fits keeps 3 planes below 4 GiB)
    float rin[C::IN_PT];
    auto load_tile = [&](int n_, int ty_, int tx_) {
        const int gy0 = ty_ * C::ROWS * S - p.pad_top, gx0 = tx_ * 32 * S - p.pad_left;
        const vcg_rsrc rx = make_rsrc(p.x + (size_t)n_ * p.cin * hw, img_bytes);
        const unsigned tb = (unsigned)gy0 * w4 + 4u * (unsigned)gx0;      // modulo 2^32 while outside the map, exact inside
        int tid_t = tid;
        if constexpr (!KEEP) asm volatile("" : "+v"(tid_t));             // a decode per tile stays one: not hoisted out of the tile loop
#pragma unroll
        for (int i = 0; i < C::IN_PT; ++i) {
            unsigned rl, q;
            if constexpr (KEEP) { rl = rel[i]; q = rc[i]; } else decode(tid_t, i, rl, q);
            bool ok = (unsigned)(gy0 + (int)(q >> 8)) < (unsigned)p.h && (unsigned)(gx0 + (int)(q & 255u)) < (unsigned)p.w_;
            if (i == C::IN_PT - 1) ok = ok && last_live;
            rin[i] = buf_load(rx, ok ? tb + rl : VCG_OOB);
        }
    };
    auto store_tile = [&](float* buf) {
#pragma unroll
        for (int i = 0; i < C::IN_PT; ++i) {
            const int e = tid + i * 256;
            if (e < C::IN_ELEMS) buf[e] = rin[i];
        }
    };
    load_tile(n, ty, tx);

    // ---- the weight slab of this block, once per workgroup: row k = (ci, tap) of element tid + 256 i is wave-uniform,
    // the lane is the output channel.  Rows past KT, channels past cin and columns past cout get VCG_OOB and read 0:
    // the row's scalar offset is added to the column's with a saturating add, so VCG_OOB stays out of range.  All
    // loads are issued before the first LDS store; flip and the (tap, ci) decode happen here only
    {
        const vcg_rsrc rwt = make_rsrc(p.w, (size_t)C::T * p.cin * p.cout * sizeof(float));
        const int wvu = __builtin_amdgcn_readfirstlane(wv);
        const unsigned col = co0 + lane < p.cout ? 4u * (unsigned)(co0 + lane) : VCG_OOB;
        float rw[C::W_PT];
#pragma unroll
        for (int i = 0; i < C::W_PT; ++i) {
            const int k = wvu + 4 * i;
            const int ci = k / C::T, tt = k % C::T;
            const int tap = p.flip ? (C::T - 1 - tt) : tt;
            const unsigned row = (k < C::KT && ci < p.cin) ? 4u * (unsigned)((tap * p.cin + ci) * p.cout) : VCG_OOB;
            rw[i] = buf_load(rwt, __builtin_elementwise_add_sat(col, row));
        }
        if (tid < 8) s_in[(tid >> 2) * C::IN_BUF + C::IN_ELEMS + (tid & 3)] = 0.f;
#pragma unroll
        for (int i = 0; i < C::W_PT; ++i) s_w[tid + i * 256] = rw[i];
    }
    store_tile(s_in);
    lds_barrier();

    const float* abase = s_w + half * 64 + l31;
    const float* b0p = s_in + (wv * 2 * S) * C::IW + l31 * S;     // lanes 0-31: k even (buffer 0)
    int cur = 0;
    for (;;) {
        // the next tile's coordinates, and its loads in flight under this tile's MFMAs
        const bool more = step < tiles - t;
        const int n0 = n, oy0 = ty * C::ROWS, ox0 = tx * 32;
        if (more) {
            t += step;
            tx += dtx;
            const int cx = tx >= p.tiles_x ? 1 : 0;
            tx -= cx ? p.tiles_x : 0;
            ty += dty + cx;
            const int cy = ty >= p.tiles_y ? 1 : 0;
            ty -= cy ? p.tiles_y : 0;
            n += dn + cy;
            load_tile(n, ty, tx);
        }

        f32x16 acc[2][2][1];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][0][r] = 0.f;

        const float* b0 = b0p + cur * C::IN_BUF;
        const float* bb1 = b0 + half * 1;                              // lanes 32-63: next tap in the row
        const float* bb2 = b0 + half * C::D_ROW;                       //              first tap of the next row
        const float* bb3 = b0 + half * C::D_CH;                        //              first tap of the next channel
        // operands are read one k-pair ahead of the MFMAs that use them, the order pinned as in conv_fwd_kernel: without
        // it hipcc gathers the reads of a short loop (4x4: 96) in front of it and spills what the tile loop carries
        auto rd = [&](int pr, float (&f)[4]) {
            const int k0 = 2 * pr, k1 = 2 * pr + 1;
            const int o0 = C::off(k0);
            const int d = (k1 < C::KT) ? (C::off(k1) - o0) : 1;       // past the end: the weight row is zero, the word read a staged value or a zero word
            const float* bb = (d == 1) ? bb1 : (d == C::D_ROW ? bb2 : bb3);
            f[0] = abase[k0 * 64];
            f[1] = abase[k0 * 64 + 32];
            f[2] = bb[o0];
            f[3] = bb[o0 + S * C::IW];
        };
        float f_[2][4];
        rd(0, f_[0]);
#pragma unroll
        for (int pr = 0; pr < C::NP; ++pr) {
            const float(&f)[4] = f_[pr & 1];
            if (pr + 1 < C::NP) rd(pr + 1, f_[(pr & 1) ^ 1]);
            acc[0][0][0] = mfma32(f[0], f[2], acc[0][0][0]);
            acc[0][1][0] = mfma32(f[0], f[3], acc[0][1][0]);
            acc[1][0][0] = mfma32(f[1], f[2], acc[1][0][0]);
            acc[1][1][0] = mfma32(f[1], f[3], acc[1][1][0]);
            if (pr + 1 < C::NP) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);   // DS reads of the next pair first
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                        // then this pair's MFMAs
        }
        // the other buffer was last read one tile ago, in front of the barrier every wave has passed since: one barrier
        // per tile.  It orders LDS only, so this tile's stores to y stay in flight under the next tile's MFMAs
        if (more) {
            store_tile(s_in + (cur ^ 1) * C::IN_BUF);
            lds_barrier();
        }
        conv_epilogue<1>(p, acc, n0, co0, oy0, ox0, wv, lane);
        if (!more) break;
        cur ^= 1;
    }
}

// ------------------------------------------------------------------------------------------------
// small-M variant (stride 1): MFMA rows = (out channel, kx); K = (in channel, ky)
// tile: 8 rows x 64 x' positions -> 64-(KW-1) valid output columns per row
// ------------------------------------------------------------------------------------------------
template <int KH, int KW, int CK>
struct SmallCfg {
    static constexpr int ROWS = 8;
    static constexpr int XW = 64;
    static constexpr int OUTW = XW - (KW - 1);
    static constexpr int IH = ROWS + KH - 1;
    static constexpr int PLANE = IH * XW;
    static constexpr int IN_ELEMS = CK * PLANE;
    static constexpr int W_ELEMS = CK * KH * 32;
    static constexpr int IN_PT = (IN_ELEMS + 255) / 256;
    static constexpr int W_PT = (W_ELEMS + 255) / 256;
    static constexpr int PST = XW + 1;                       // scratch row stride
    static constexpr int SCRATCH = 4 * 32 * PST;             // one 32 x 64 tile per wave
    static constexpr int LDS_ELEMS = (IN_ELEMS + W_ELEMS) > SCRATCH ? (IN_ELEMS + W_ELEMS) : SCRATCH;
    static constexpr size_t LDS_BYTES = (size_t)LDS_ELEMS * sizeof(float);
};

template <int KH, int KW, int CK>
__global__ __launch_bounds__(256) void conv_smallm_kernel(const ConvParams p) {
    using C = SmallCfg<KH, KW, CK>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_in = smem;               // [CK][IH][64]
    float* s_w = smem + C::IN_ELEMS;  // [CK][KH][32]   (row mi = mch*KW + kx)

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    int b = blockIdx.x;
    const int tx = b % p.tiles_x; b /= p.tiles_x;
    const int ty = b % p.tiles_y; b /= p.tiles_y;
    const int n = b;
    const int ox0 = tx * C::OUTW, oy0 = ty * C::ROWS;
    const int gy0 = oy0 - p.pad_top, gx0 = ox0 - p.pad_left;
    const float* xn = p.x + (size_t)n * p.cin * p.h * p.w_;
    const int mrows = p.cout * KW;

    float rin[C::IN_PT], rw[C::W_PT];
    // the staged rows are exactly 64 floats wide: row (ci, r) is wave-uniform and the lane is the column,
    // so the input addressing is scalar + lane
    const int wvu = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int gx = gx0 + lane;
    const bool col_ok = gx >= 0 && gx < p.w_;
    const int gxc = min(max(gx, 0), p.w_ - 1);
    const int hw = p.h * p.w_;
    // range-checked buffer loads: padding / missing channels get the offset VCG_OOB and read as 0 (vcg_common.hpp)
    const vcg_rsrc rx = make_rsrc(xn, (size_t)p.cin * hw * sizeof(float));
    const vcg_rsrc rwt = make_rsrc(p.w, (size_t)KH * KW * p.cin * p.cout * sizeof(float));
    auto load_chunk = [&](int ci0) {
#pragma unroll
        for (int i = 0; i < C::IN_PT; ++i) {
            const int q = wvu + 4 * i;                  // row index inside the chunk tile
            const int r = q % C::IH, ci = q / C::IH;
            const int gy = gy0 + r, ch = ci0 + ci;
            const bool ok = col_ok && ch < p.cin && gy >= 0 && gy < p.h;
            rin[i] = buf_load(rx, ok ? 4u * (unsigned)(ch * hw + gy * p.w_ + gxc) : VCG_OOB);
        }
#pragma unroll
        for (int i = 0; i < C::W_PT; ++i) {
            const int e = tid + i * 256;
            const int mi = e & 31, q = e >> 5;
            const int ky = q % KH, ci = q / KH;
            const int ch = ci0 + ci;
            const bool ok = e < C::W_ELEMS && ch < p.cin && mi < mrows;
            const int mch = mi / KW, kx = mi % KW;
            int tap = ky * KW + kx;
            if (p.flip) tap = KH * KW - 1 - tap;
            rw[i] = buf_load(rwt, ok ? 4u * (unsigned)(tap * p.ws_t + mch * p.ws_m + ch * p.ws_k) : VCG_OOB);
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < C::IN_PT; ++i) {
            const int e = tid + i * 256;
            if (e < C::IN_ELEMS) s_in[e] = rin[i];
        }
#pragma unroll
        for (int i = 0; i < C::W_PT; ++i) {
            const int e = tid + i * 256;
            if (e < C::W_ELEMS) s_w[e] = rw[i];
        }
    };

    f32x16 acc[2][2];  // [row tile][x tile]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const float* bbase = s_in + half * C::PLANE + (wv * 2) * C::XW + l31;
    const float* abase = s_w + half * KH * 32 + l31;

    const int nchunks = (p.cin + CK - 1) / CK;
    load_chunk(0);
    for (int c = 0; c < nchunks; ++c) {
        __syncthreads();
        store_chunk();
        __syncthreads();
        if (c + 1 < nchunks) load_chunk((c + 1) * CK);
#pragma unroll
        for (int cp = 0; cp < CK / 2; ++cp) {
#pragma unroll
            for (int ky = 0; ky < KH; ++ky) {
                const float a = abase[(cp * 2 * KH + ky) * 32];
                const float b00 = bbase[cp * 2 * C::PLANE + ky * C::XW];
                const float b01 = bbase[cp * 2 * C::PLANE + ky * C::XW + 32];
                const float b10 = bbase[cp * 2 * C::PLANE + (ky + 1) * C::XW];
                const float b11 = bbase[cp * 2 * C::PLANE + (ky + 1) * C::XW + 32];
                acc[0][0] = mfma32(a, b00, acc[0][0]);
                acc[0][1] = mfma32(a, b01, acc[0][1]);
                acc[1][0] = mfma32(a, b10, acc[1][0]);
                acc[1][1] = mfma32(a, b11, acc[1][1]);
            }
        }
    }

    // epilogue: out[mch][x] = sum_kx P[mch*KW+kx][x+kx]; one output row at a time through LDS
    float* s_p = smem + wv * 32 * C::PST;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        __syncthreads();  // staging LDS (or previous scratch) no longer read by anyone
#pragma unroll
        for (int xt = 0; xt < 2; ++xt)
#pragma unroll
            for (int r = 0; r < 16; ++r) s_p[mfma_row(r, lane) * C::PST + xt * 32 + l31] = acc[rt][xt][r];
        __syncthreads();
        const int oy = oy0 + wv * 2 + rt;
        const int ox = ox0 + lane;
        if (lane < C::OUTW && oy < p.oh && ox < p.ow) {
            for (int mch = 0; mch < p.cout; ++mch) {
                float v = 0.f;
#pragma unroll
                for (int kx = 0; kx < KW; ++kx) v += s_p[(mch * KW + kx) * C::PST + lane + kx];
                const float bv = p.bias ? p.bias[mch] : 0.f;
                const float al = (p.act == VCG_ACT_PRELU) ? p.prelu[mch] : p.alpha;
                const size_t idx = (((size_t)n * p.cout + mch) * p.oh + oy) * p.ow + ox;
                v = apply_act(v + bv, p.act, al);
                if (p.residual) v += p.residual[idx];
                p.y[idx] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// one output channel, stride 1 (the PatchGAN head: Conv2D(1, 4) on 512 channels): 0.5 GFLOP over 65 MB of input -- memory
// work, not matrix work.  On the small-M MFMA kernel it occupies 4 of an MFMA's 32 rows and is bound by the wasted rows
// (0.32 ms); here it is a plain FMA reduction: block = (image, output row, 64 columns), wave = a quarter of the input
// channels, lane = column; the K shifted loads of a row overlap in L1; the four partial sums meet in LDS in a fixed order.
// ------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(256) void conv_cout1_kernel(const ConvParams p) {
    __shared__ float red[4][64];
    const int tid = threadIdx.x, xl = tid & 63;
    const int cg = __builtin_amdgcn_readfirstlane(tid >> 6);
    int b = blockIdx.x;
    const int seg = b % p.tiles_x; b /= p.tiles_x;
    const int oy = b % p.oh;
    const int n = b / p.oh;
    const int ox = seg * 64 + xl, gx0 = ox - p.pad_left, gy0 = oy - p.pad_top;
    const int hw = p.h * p.w_;
    const vcg_rsrc rx = make_rsrc(p.x + (size_t)n * p.cin * hw, (size_t)p.cin * hw * sizeof(float));
    unsigned coff[K];                                            // byte offset of (row 0, column gx0 + kx) or out of range
#pragma unroll
    for (int kx = 0; kx < K; ++kx) coff[kx] = (unsigned)(gx0 + kx) < (unsigned)p.w_ ? 4u * (unsigned)(gx0 + kx) : VCG_OOB;
    float acc = 0.f;
#pragma unroll 1                                                 // (unrolled x4 hipcc makes it 3x slower)
    for (int c = cg; c < p.cin; c += 4) {
        float wr[K * K];
#pragma unroll
        for (int t = 0; t < K * K; ++t) wr[t] = p.w[(p.flip ? K * K - 1 - t : t) * p.ws_t + c * p.ws_k];       // wave-uniform: scalar loads
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int gy = gy0 + ky;
            const bool rok = (unsigned)gy < (unsigned)p.h;
            const unsigned rbase = 4u * (unsigned)(c * hw + gy * p.w_);
#pragma unroll
            for (int kx = 0; kx < K; ++kx) acc += buf_load(rx, rok && coff[kx] != VCG_OOB ? rbase + coff[kx] : VCG_OOB) * wr[ky * K + kx];
        }
    }
    red[cg][xl] = acc;
    __syncthreads();
    if (cg == 0 && ox < p.ow) {
        float v = ((red[0][xl] + red[1][xl]) + (red[2][xl] + red[3][xl])) + (p.bias ? p.bias[0] : 0.f);
        if (p.act == VCG_ACT_LRELU) v = v >= 0.f ? v : v * p.alpha;
        else if (p.act == VCG_ACT_TANH) v = tanhf(v);
        const size_t o = ((size_t)n * p.oh + oy) * p.ow + ox;
        if (p.residual) v += p.residual[o];
        p.y[o] = v;
    }
}

template <int K>
int launch_cout1(ConvParams p, hipStream_t st) {
    p.tiles_x = ceil_div(p.ow, 64);
    const long grid = (long)p.tiles_x * p.oh * p.n;
    if (grid <= 0 || grid > 0x7fffffffL) return VCG_E_SHAPE;
    hipLaunchKernelGGL(conv_cout1_kernel<K>, dim3((unsigned)grid), dim3(256), 0, st, p);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

template <typename Kern>
int launch_with_lds(Kern kern, int grid, size_t lds, const ConvParams& p, hipStream_t st) {
    if (int e = vcg_allow_dyn_lds(reinterpret_cast<const void*>(kern), lds)) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, p);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

// conv_epilogue addresses the (image, 64-channel block) of y it writes through one buffer descriptor with 32-bit byte
// offsets: all 64 rows of the tile form one, the rows past cout included (they must land behind num_records, not wrap
// around), so 64 planes must stay below the descriptor's 0xFFFFFFE0 ceiling; the staging loads a chunk of ck input
// planes likewise
bool conv_block_fits(int oh, int ow, int ck, int h, int w) {
    const unsigned long long lim = 0xFFFFFFE0ull;
    return 64ull * oh * ow * sizeof(float) < lim && (unsigned long long)ck * h * w * sizeof(float) < lim;
}

template <int KH, int KW, int S, int CK, int XT>
int launch_conv(ConvParams p, hipStream_t st) {
    using C = ConvCfg<KH, KW, S, CK, XT>;
    if (!conv_block_fits(p.oh, p.ow, CK, p.h, p.w_)) return VCG_E_UNSUPPORTED;
    p.tiles_x = ceil_div(p.ow, 32 * XT);
    p.tiles_y = ceil_div(p.oh, C::ROWS);
    p.co_blocks = ceil_div(p.cout, 64);
    const long grid = (long)p.tiles_x * p.tiles_y * p.co_blocks * p.n;
    if (grid <= 0 || grid > 0x7fffffffL) return VCG_E_SHAPE;
    if (p.stats && p.scale) return VCG_E_UNSUPPORTED;
    if (p.stats) {
        // instantiated for the layers a normalisation follows in the fp32 configs: the trunk's 3x3 and the critics' 3x3 / 4x4 stride 1 and 2
        if constexpr ((KH == 3 && KW == 3 && S <= 2) || (KH == 4 && KW == 4 && S <= 2))
            return launch_with_lds(conv_fwd_kernel<KH, KW, S, CK, XT, true>, (int)grid, C::LDS_BYTES, p, st);
        else
            return VCG_E_UNSUPPORTED;
    }
    // the affine epilogue is instantiated for the stride-1 3x3 / 5x5 layers (the generators' trunks)
    if (p.scale) {
        if constexpr (S == 1 && ((KH == 3 && KW == 3) || (KH == 5 && KW == 5)))
            return launch_with_lds(conv_fwd_kernel<KH, KW, S, CK, XT, false, true>, (int)grid, C::LDS_BYTES, p, st);
        else
            return VCG_E_UNSUPPORTED;
    }
    return launch_with_lds(conv_fwd_kernel<KH, KW, S, CK, XT>, (int)grid, C::LDS_BYTES, p, st);
}

// compute units of the device, asked once (the devices of one process are alike); 0 if the runtime cannot say
int device_cu_count() {
    static const int cus = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        return v;
    }();
    return cus;
}

template <int KH, int KW, int S>
int launch_c3(ConvParams p, hipStream_t st) {
    using C = C3Cfg<KH, KW, S>;
    if (!conv_block_fits(p.oh, p.ow, 3, p.h, p.w_)) return VCG_E_UNSUPPORTED;
    p.tiles_x = ceil_div(p.ow, 32);
    p.tiles_y = ceil_div(p.oh, C::ROWS);
    p.co_blocks = ceil_div(p.cout, 64);
    const long tiles = (long)p.tiles_x * p.tiles_y * p.co_blocks * p.n;
    if (tiles <= 0 || tiles > 0x7fffffffL) return VCG_E_SHAPE;
    // persistent: two workgroups per CU (the kernel's launch bounds), a whole number of them per channel block
    const int cus = device_cu_count();
    if (cus <= 0) return VCG_E_UNSUPPORTED;
    long grid = tiles < 2L * cus ? tiles : 2L * cus;
    grid -= grid % p.co_blocks;
    if (grid < p.co_blocks) grid = p.co_blocks;
    return launch_with_lds(conv_c3_kernel<KH, KW, S>, (int)grid, C::LDS_BYTES, p, st);
}

template <int KH, int KW, int CK>
int launch_smallm(ConvParams p, hipStream_t st) {
    using C = SmallCfg<KH, KW, CK>;
    p.tiles_x = ceil_div(p.ow, C::OUTW);
    p.tiles_y = ceil_div(p.oh, C::ROWS);
    p.co_blocks = 1;
    const long grid = (long)p.tiles_x * p.tiles_y * p.n;
    if (grid <= 0 || grid > 0x7fffffffL) return VCG_E_SHAPE;
    return launch_with_lds(conv_smallm_kernel<KH, KW, CK>, (int)grid, C::LDS_BYTES, p, st);
}

}  // namespace

// conv_rowchain.hip: 9x9, 256 -> <=3 channels, width % 64 == 0 (the generator's final/conv); VCG_E_UNSUPPORTED otherwise
int vcg_internal_conv9_rowchain(const float* x, const float* w, float* y, int n, int cin, int h, int wd, int cout, const float* bias, int act,
                                int ws_t, int ws_m, int ws_k, hipStream_t st);

// Generic entry used by the C ABI wrappers in api.hip.  Weight tensor w is [T][cin][cout] with cout
// contiguous (or addressed by ws_* strides for the small-M kernel).
int vcg_internal_conv(const float* x, const float* w, float* y, int n, int cin, int h, int wd, int cout,
                      int oh, int ow, int kh, int kw, int stride, int pad_top, int pad_left, int flip,
                      const vcg_epilogue* ep, int smallm, int ws_t, int ws_m, int ws_k, hipStream_t st, float* stats, const float* scale, const float* shift) {
    ConvParams p{};
    p.x = x; p.w = w; p.y = y; p.stats = stats;
    if (stats && (smallm || cin <= 3)) return VCG_E_UNSUPPORTED;
    // scale / shift: the affine stage exists in conv_fwd_kernel's epilogue only (conv_c3_kernel<9,9,1> has no register to spare for it)
    if (scale && (smallm || stats || cin <= 3)) return VCG_E_UNSUPPORTED;
    if (scale && shift == nullptr) return VCG_E_NULL;
    p.scale = scale; p.shift = scale ? shift : nullptr;
    p.bias = ep ? ep->bias : nullptr;
    p.prelu = ep ? ep->prelu_alpha : nullptr;
    p.residual = ep ? ep->residual : nullptr;
    p.act = ep ? ep->act : VCG_ACT_NONE;
    p.alpha = ep ? ep->act_alpha : 0.f;
    if (p.act == VCG_ACT_PRELU && p.prelu == nullptr) return VCG_E_NULL;
    p.n = n; p.cin = cin; p.h = h; p.w_ = wd; p.cout = cout; p.oh = oh; p.ow = ow;
    p.pad_top = pad_top; p.pad_left = pad_left; p.flip = flip;
    p.ws_t = ws_t; p.ws_m = ws_m; p.ws_k = ws_k;
    if (n <= 0 || cin <= 0 || cout <= 0 || oh <= 0 || ow <= 0) return VCG_E_SHAPE;
    if (smallm) {
        if (stride != 1 || cout * kw > 32) return VCG_E_UNSUPPORTED;
        if (kh == 9 && kw == 9 && !flip && pad_top == 4 && pad_left == 4 && oh == h && ow == wd && !p.prelu && !p.residual) {
            const int rc = vcg_internal_conv9_rowchain(x, w, y, n, cin, h, wd, cout, p.bias, p.act, ws_t, ws_m, ws_k, st);
            if (rc != VCG_E_UNSUPPORTED) return rc;
        }
        // one output channel on many input channels: the FMA reduction (the MFMA rows of the small-M kernel would be 7/8 padding)
        if (cout == 1 && cin >= 64 && kh == kw && ws_m == 1 && !p.prelu && (size_t)cin * h * wd * 4 <= 0xFFFFFFE0u) {
            if (kh == 3) return launch_cout1<3>(p, st);
            if (kh == 4) return launch_cout1<4>(p, st);
            if (kh == 5) return launch_cout1<5>(p, st);
        }
        if (kh == 9 && kw == 9) return launch_smallm<9, 9, 8>(p, st);
        if (kh == 4 && kw == 4) return launch_smallm<4, 4, 8>(p, st);
        if (kh == 3 && kw == 3) return launch_smallm<3, 3, 8>(p, st);
        if (kh == 5 && kw == 5) return launch_smallm<5, 5, 8>(p, st);
        return VCG_E_UNSUPPORTED;
    }
    if (p.act == VCG_ACT_TANH) return VCG_E_UNSUPPORTED;   // tanh epilogue: small-M kernel only (<= 32/kw channels)
    if (cin <= 3) {   // flat-K kernel: no channel padding (first conv on RGB, data gradient of a 3-channel conv)
        if (kh == 9 && kw == 9 && stride == 1) return launch_c3<9, 9, 1>(p, st);
        if (kh == 3 && kw == 3 && stride == 1) return launch_c3<3, 3, 1>(p, st);
        if (kh == 4 && kw == 4 && stride == 2) return launch_c3<4, 4, 2>(p, st);
        if (kh == 5 && kw == 5 && stride == 1) return launch_c3<5, 5, 1>(p, st);     // sparse_512 block 1 (model.py:967)
    }
    // wide outputs use 64-column tiles (two MFMA x-tiles per wave: half the barriers and weight staging per
    // MFMA, and 1024 workgroups = 2 full rounds of 2 per CU at the C2 trunk shape instead of 2.67 rounds of 3)
    const bool wide = ow > 32;
    if (kh == 3 && kw == 3 && stride == 1) return wide ? launch_conv<3, 3, 1, 8, 2>(p, st) : launch_conv<3, 3, 1, 8, 1>(p, st);
    if (kh == 5 && kw == 5 && stride == 1) return launch_conv<5, 5, 1, 8, 1>(p, st);   // XT=2 spills (50 weight prefetch registers)
    if (scale) return VCG_E_UNSUPPORTED;                     // every other instantiation: see launch_conv
    if (kh == 3 && kw == 3 && stride == 2) return launch_conv<3, 3, 2, 8, 1>(p, st);
    if (kh == 4 && kw == 4 && stride == 1) return launch_conv<4, 4, 1, 8, 1>(p, st);   // XT=2 spills here (measured slower)
    if (kh == 4 && kw == 4 && stride == 2) return launch_conv<4, 4, 2, 4, 1>(p, st);
    if (kh == 5 && kw == 5 && stride == 2) return launch_conv<5, 5, 2, 4, 1>(p, st);
    if (kh == 5 && kw == 5 && stride == 3) return launch_conv<5, 5, 3, 4, 1>(p, st);   // sparse_512 blocks 2-6 (model.py:971-987)
    if (kh == 9 && kw == 9 && stride == 1) return launch_conv<9, 9, 1, 4, 1>(p, st);
    // make_upscaler_incep_resnet (model.py:372-440): 1x1, and the 1xk / kx1 pairs of the 2-path blocks (and their data gradients)
    if (stride == 1) {
        if (kh == 1 && kw == 1) return launch_conv<1, 1, 1, 8, 1>(p, st);
        if (kh == 1 && kw == 3) return launch_conv<1, 3, 1, 8, 1>(p, st);
        if (kh == 3 && kw == 1) return launch_conv<3, 1, 1, 8, 1>(p, st);
        if (kh == 1 && kw == 5) return launch_conv<1, 5, 1, 8, 1>(p, st);
        if (kh == 5 && kw == 1) return launch_conv<5, 1, 1, 8, 1>(p, st);
        if (kh == 1 && kw == 7) return launch_conv<1, 7, 1, 8, 1>(p, st);
        if (kh == 7 && kw == 1) return launch_conv<7, 1, 1, 8, 1>(p, st);
    }
    return VCG_E_UNSUPPORTED;
}
