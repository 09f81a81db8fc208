// bf16 3x3 trunk convolution (64 -> 64 channels, v1 and v2) and the convolutions on three input channels (gates included): kernels,
// launch helpers and C entry points.  Two families in one translation unit on purpose: conv3x3_c64_bf16_v2_kernel<.., STATS> and
// conv_c3to64_bf16_kernel both call half_wave_reduce_scatter32, and the compiler propagates argument ranges between functions before it
// applies forced inlining, so with either caller in a file of its own the ungated conv_c3to64_bf16_kernel instantiations come out with
// another register allocation (scripts/device_isa.py --per-kernel shows it).  Split them only together with a per-kernel timing.
#include "bf16_tiles.hpp"
#include "vcg_stamps.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// 3x3 stride-1 'same' convolution, 64 -> 64 channels: the generator trunk
// ---------------------------------------------------------------------------------------------------------------
// At bf16 this convolution is HBM-bound even at the full MFMA rate (per 16x32 pixels: 142 KB of traffic against
// 9.2 k MFMA cycles per SIMD), so the kernel is organised around keeping loads AND stores in flight under the MFMAs:
//   * persistent workgroups of 8 waves: 6 compute waves + 2 loader waves (wave-specialised: vmcnt is per wave
//     and retires in order, so a wave that both prefetches and stores ends up draining its stores before it may
//     touch the prefetched registers; with the roles split, neither side ever waits for the other's traffic);
//   * LDS: all 9x64x64 weights (72 KiB, loaded once) + one 14x34-pixel halo tile (59.5 KiB) + 768 B of epilogue
//     parameters.  Both images hold 128-byte rows (one pixel / one out-channel x 64 in-channels) whose eight 16-byte
//     chunks are XOR-swizzled with (index>>1)&7: the ds_read_b128 of the 16-lane groups {0-3,12-15,20-27},
//     {4-11,16-19,28-31} (MI355X_MICROARCH.md, LDS) then touches all 64 banks once, for every tap shift;
//   * compute wave w owns output rows 2w, 2w+1 of the 12x32 tile: a 64-channel x 64-pixel accumulator (4 MFMA tiles,
//     64 VGPRs), operand fragments double-buffered in registers (reads of k-step i+1 issued before the MFMAs of i);
//   * loader waves fetch the next tile's halo into registers during the MFMA phase and write it to LDS between the
//     two barriers that end a tile, while the compute waves run their epilogue.
// (NCW, NLW, TR, TC, HR, HC, ROWB, WB, NT: bf16_tiles.hpp)
constexpr int XB = HR * ROWB;               // 60928
constexpr int PB = 3 * 64 * 4;              // per-channel epilogue parameters: scale, shift, negative-side slope
constexpr int NCHUNK = HR * HC * 8;         // 16-byte chunks per halo tile (3808)
constexpr int NPRE = (NCHUNK + NLW * 64 - 1) / (NLW * 64);   // per-loader-thread prefetch registers (30)

struct C3Params {
    const uint4* x;
    const uint4* w;
    __bf16* y;
    const float* scale;
    const float* shift;
    const float* alpha;
    const __bf16* res;
    int n, h, w_, tiles_x, tiles_y, total;
    int act;
    float act_alpha;
    float* stats;            // v2 with STATS: per-channel sum / sum of squares of the stored (bf16-rounded) output, [unit][row group][2][64]
    int stats_per_tile;      // 0: unit = workgroup (one record pair per launch: batch statistics); 1: unit = tile (instance norm)
};

template <bool AFF, bool SLOPE, bool RES>
__global__ __launch_bounds__(NT, 1) void conv3x3_c64_bf16_kernel(C3Params p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* wl = smem;
    unsigned char* xl = smem + WB;
    float* prm = (float*)(smem + WB + XB);
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);

    for (int c = tid; c < 9 * 64 * 8; c += NT) {
        const int chunk = c & 7, co = (c >> 3) & 63, tap = c >> 9;
        *(uint4*)(wl + tap * 8192 + co * 128 + ((chunk ^ ((co >> 1) & 7)) << 4)) = p.w[c];
    }
    if (tid < 64) {
        prm[tid] = p.scale ? p.scale[tid] : 1.f;
        prm[64 + tid] = p.shift ? p.shift[tid] : 0.f;
        prm[128 + tid] = p.act == VCG_ACT_PRELU ? p.alpha[tid] : (p.act == VCG_ACT_LRELU ? p.act_alpha : 1.f);
    }

    if (wv >= NCW) {
        // ------------------------------------------------------------------------------------------ loader waves
        const int lt = tid - NCW * 64;
        uint4 pre[NPRE];
        unsigned okmask = 0;
        auto fetch = [&](int tile) {
            const int txi = tile % p.tiles_x, t2 = tile / p.tiles_x, tyi = t2 % p.tiles_y, img = t2 / p.tiles_y;
            const int y0 = tyi * TR - 1, x0 = txi * TC - 1;
            okmask = 0;
#pragma unroll
            for (int i = 0; i < NPRE; ++i) {
                const int c = min(lt + NLW * 64 * i, NCHUNK - 1);     // the tail re-reads the last chunk: same data, same slot
                const int pix = c >> 3, row = pix / HC, col = pix - row * HC;
                const int gy = y0 + row, gx = x0 + col;
                const bool ok = (unsigned)gy < (unsigned)p.h && (unsigned)gx < (unsigned)p.w_;
                const int cy = min(max(gy, 0), p.h - 1), cx = min(max(gx, 0), p.w_ - 1);
                pre[i] = p.x[((long)(img * p.h + cy) * p.w_ + cx) * 8 + (c & 7)];
                okmask |= ok ? (1u << i) : 0u;
            }
        };
        auto stash = [&]() {
#pragma unroll
            for (int i = 0; i < NPRE; ++i) {
                const int c = min(lt + NLW * 64 * i, NCHUNK - 1);
                const int pix = c >> 3, row = pix / HC, col = pix - row * HC;
                const uint4 v = (okmask >> i) & 1u ? pre[i] : make_uint4(0, 0, 0, 0);
                *(uint4*)(xl + pix * 128 + (((c & 7) ^ ((col >> 1) & 7)) << 4)) = v;
            }
        };
        int tile = blockIdx.x;
        fetch(tile);
        stash();
        lds_barrier();                                   // B0: weights, parameters and the first tile are in LDS
        for (; tile < p.total; tile += gridDim.x) {
            const int next = tile + gridDim.x;
            if (next < p.total) fetch(next);
            lds_barrier();                               // A: the compute waves have read the current tile
            if (next < p.total) stash();
            lds_barrier();                               // B: the next tile is in LDS
        }
        return;
    }

    // --------------------------------------------------------------------------------------------- compute waves
    int aoff[4], boff[3][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) aoff[s] = r * 128 + (((2 * s + hh) ^ ((r >> 1) & 7)) << 4);
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int pos = r + dx;
            boff[dx][s] = pos * 128 + (((2 * s + hh) ^ ((pos >> 1) & 7)) << 4);
        }
    const unsigned char* xb = xl + (wv * 2) * ROWB;
    lds_barrier();                                       // B0

    for (int tile = blockIdx.x; tile < p.total; tile += gridDim.x) {
        const int txi = tile % p.tiles_x, t2 = tile / p.tiles_x, tyi = t2 % p.tiles_y, img = t2 / p.tiles_y;
        const int gx = txi * TC + r, gy0 = tyi * TR + wv * 2;
        const bool okx = gx < p.w_;

        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

        // 36 k-steps (9 taps x 4 channel groups of 16)
        bf16x8 fa[2][2], fb[2][2];
        bf16x8 rr[2][2][2];
        // k-step at which the residual tile is requested: under the last 8 k-steps.  Requesting it at k-step 3 (under 32 k-steps, to cover a
        // whole HBM round trip) measured SLOWER: 73 against 61 us (data gradient + skip) and 57.6 against 55.6 us at batch 8, 194.5 against 190
        // at batch 32 -- VCG_RES_AT re-defines it for A/B builds
#ifndef VCG_RES_AT
#define VCG_RES_AT 27
#endif
        constexpr int RES_AT = VCG_RES_AT;
        auto frag = [&](int i, int buf) {
            const int tap = i >> 2, s = i & 3, dy = tap / 3, dx = tap - 3 * dy;
            const unsigned char* wa = wl + tap * 8192 + aoff[s];
            fa[buf][0] = *(const bf16x8*)(wa);
            fa[buf][1] = *(const bf16x8*)(wa + 4096);
            fb[buf][0] = *(const bf16x8*)(xb + dy * ROWB + boff[dx][s]);
            fb[buf][1] = *(const bf16x8*)(xb + (dy + 1) * ROWB + boff[dx][s]);
        };
        frag(0, 0);
#pragma unroll
        for (int i = 0; i < 36; ++i) {
            const int cur = i & 1;
            if (i + 1 < 36) frag(i + 1, cur ^ 1);
            __builtin_amdgcn_sched_barrier(0);          // keep the next step's reads ahead of this step's MFMAs
            acc[0][0] = mfma_bf16(fa[cur][0], fb[cur][0], acc[0][0]);
            acc[0][1] = mfma_bf16(fa[cur][0], fb[cur][1], acc[0][1]);
            acc[1][0] = mfma_bf16(fa[cur][1], fb[cur][0], acc[1][0]);
            acc[1][1] = mfma_bf16(fa[cur][1], fb[cur][1], acc[1][1]);
            __builtin_amdgcn_sched_barrier(0);
            if (i == RES_AT && RES) {
                // the residual tile: requested under the remaining k-steps, 16 bytes (8 channels) per lane and group
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int q = 0; q < 2; ++q)
#pragma unroll
                        for (int pt = 0; pt < 2; ++pt) {
                            const int cy = min(gy0 + pt, p.h - 1), cx = min(gx, p.w_ - 1);
                            rr[mt][q][pt] = *(const bf16x8*)(p.res + ((long)(img * p.h + cy) * p.w_ + cx) * 64 + mt * 32 + 16 * q + 8 * hh);
                        }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        lds_barrier();                                   // A: this tile's LDS image may be overwritten

        // epilogue: y = act(acc * scale + shift) + residual -> bf16.  An MFMA tile leaves lane (pixel, h) with channels
        // 8g+4h+{0..3}; v_permlane32_swap between the register groups (2q, 2q+1) of the two half-waves turns that into
        // 8 consecutive channels 16q+8h+{0..7}: 16-byte residual loads and stores.  Phase 1 computes all final values
        // (consuming every outstanding load), phase 2 is nothing but the 8 stores, which then drain under the next
        // tile's MFMAs.
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int co = mt * 32 + 16 * q + 8 * hh;
                float sc[8], sh[8], al[8];
                if (AFF) {
                    *(f32x4*)&sc[0] = *(const f32x4*)(prm + co);
                    *(f32x4*)&sc[4] = *(const f32x4*)(prm + co + 4);
                    *(f32x4*)&sh[0] = *(const f32x4*)(prm + 64 + co);
                    *(f32x4*)&sh[4] = *(const f32x4*)(prm + 64 + co + 4);
                }
                if (SLOPE) {
                    *(f32x4*)&al[0] = *(const f32x4*)(prm + 128 + co);
                    *(f32x4*)&al[4] = *(const f32x4*)(prm + 128 + co + 4);
                }
#pragma unroll
                for (int pt = 0; pt < 2; ++pt) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float lo = acc[mt][pt][8 * q + j], hi = acc[mt][pt][8 * q + 4 + j];
                        swap32(lo, hi);
                        v[j] = lo;
                        v[4 + j] = hi;
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float u = v[j];
                        if (AFF) u = u * sc[j] + sh[j];
                        if (SLOPE) u = u >= 0.f ? u : u * al[j];
                        if (RES) u += (float)rr[mt][q][pt][j];
                        acc[mt][pt][8 * q + j] = u;
                    }
                }
            }
        // pin phase 1 here (otherwise its arithmetic is sunk into the conditional store blocks, and with it the waits)
        asm volatile("" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[1][0]), "+v"(acc[1][1]));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int pt = 0; pt < 2; ++pt) {
                    bf16x8 ov;
#pragma unroll
                    for (int j = 0; j < 8; ++j) ov[j] = (__bf16)acc[mt][pt][8 * q + j];
                    const int gy = gy0 + pt;
                    if (gy < p.h && okx) *(bf16x8*)(p.y + ((long)(img * p.h + gy) * p.w_ + gx) * 64 + mt * 32 + 16 * q + 8 * hh) = ov;
                }
        lds_barrier();                                   // B: the next tile is in LDS
    }
}

// ---------------------------------------------------------------------------------------------------------------
// v2 of the trunk convolution: weights in REGISTERS, halo tiles double-buffered by LDS-DMA, one wave per SIMD
// ---------------------------------------------------------------------------------------------------------------
// v1 keeps all 9x64x64 weights in LDS (72 KiB), which leaves room for ONE halo tile: hence its loader waves, its two
// barriers per tile, the 2+1+1+2 placement of six compute waves on four SIMDs and one LDS read per MFMA.  Here the
// workgroup is four waves, one per SIMD, each with the 512-register budget that buys:
//   * a wave owns 32 of the 64 output channels x 8 of the 16 tile rows and keeps ITS 36 weight fragments (9 taps x 4
//     channel groups) in 144 registers for the whole launch -- no weights in LDS at all;
//   * LDS holds two 18x34-pixel halo tiles (2 x 76.5 KiB), filled by `buffer_load_dwordx4 ... lds` (range-checked by the
//     buffer descriptor: the zero padding costs no branch and no select on data);
//   * a software pipeline over HALF tiles (two accumulator sets of 4 rows): the epilogue of one half is issued in the MFMA
//     shadow of the other, the next tile's DMA pieces in phase A's -- see the tile loop;
//   * one barrier per tile; it orders LDS only, so the stores drain under the following MFMAs.
// Measured (scripts/micro/stamps.py run v2, batch 32 at 256x256, sustained): 13.6 k cycles per tile for 9.2 k of MFMA issue
// (serial epilogue: 15.4 k; v1's pipe is busy 28 % of the time) at the 1.6 GHz the chip holds under this load -- a bare
// v_mfma_f32_32x32x16_bf16 stream on random operands holds 1.5-1.75 GHz = 1.5-1.75 PFLOP/s (scripts/micro/mfma_peak_bf16.hip):
// the kernel is power-limited, and cycles saved come back as a lower clock.  The variant WITH a
// residual input stays on v1: it moves 1.5x the bytes, and with one wave per SIMD every stalled vector-memory issue also
// stalls that SIMD's MFMA stream (measured 0.234 ms against 0.213).
constexpr int V2_TR = 16, V2_TC = 32, V2_HR = V2_TR + 2, V2_HC = V2_TC + 2;
constexpr int V2_ROWB = V2_HC * 128;
constexpr int V2_XB = V2_HR * V2_ROWB;                          // 78336
constexpr int V2_NT = 256;
constexpr int V2_CHUNKS = V2_XB / 16;                           // 4896 = 19 * 256 + 32
constexpr int V2_NDMA = (V2_CHUNKS + V2_NT - 1) / V2_NT;        // 20 rounds; the last one is half of wave 0
constexpr int V2_PAD = 512;                                     // what the other half of that wave writes (zeros) past the tile
constexpr int V2_BUF = V2_XB + V2_PAD;
constexpr int V2_LDS = 2 * V2_BUF + PB;
static_assert(V2_LDS <= 160 * 1024, "v2 trunk kernel: LDS");
static_assert(V2_NDMA == 20 && V2_CHUNKS - 19 * V2_NT == 32, "v2 trunk kernel: DMA schedule");

// (namespace scope: hipcc emits no host stub for a kernel template whose lambdas return a struct local to the kernel)
struct TileSrc { unsigned base; int x0; vcg_rsrc rs; };          // a tile's halo: byte offset of its origin in the image, first column, image descriptor
struct OutPos { vcg_rsrc rs; int gx, gy0; bool okx; };           // where a half's accumulators go: image descriptor, column, first row

// Diagnostic build only (-DVCG_STAMPS, scripts/micro/stamps.py): s_memtime brackets around the four segments of a
// tile, summed per wave in scalar registers and written to a buffer of their own after the loop: [256 workgroups][4 waves][phase A,
// phase B, vmcnt wait, barrier, kernel core clocks, kernel 100-MHz ticks].  No stamp executes in
// the shipped library; read the SHARES of such a build, not its run time (cdna_hip_programming.md, In-kernel stamps).
VCG_STAMP_SUMS(v2, 256 * 4 * 6);

// STATS: the epilogue also accumulates, per lane, the sum and the sum of squares of the values it stores (as rounded to bf16: the
// statistics are those of the tensor the next kernel reads) for the training-mode BatchNormalization / instance norm behind the
// convolution (model.py:20,23,284) -- the separate statistics pass over the output (one more read of the tensor, two more launches
// per normalisation) is gone.  16 values of a store unit cost 24 vector instructions in two more stages of the drain; the 32 partial
// sums of a lane are reduced over the 32 pixels of the wave once per launch (once per tile for per-image statistics) and written as
// one record per (workgroup | tile, row group); vcg_norm_finalize_partials sums the records in a fixed order.
template <bool AFF, bool SLOPE, bool STATS = false>
__global__ __launch_bounds__(V2_NT, 1) void conv3x3_c64_bf16_v2_kernel(C3Params p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#ifdef VCG_STAMPS
    const unsigned long long k_c0 = __builtin_amdgcn_s_memtime(), k_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    float* prm = (float*)(smem + 2 * V2_BUF);
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int coh = wv & 1, rg = wv >> 1;                       // channel half, row group (rows 8rg .. 8rg+7 of the tile)

    if (tid < 64) {
        prm[tid] = p.scale ? p.scale[tid] : 1.f;
        prm[64 + tid] = p.shift ? p.shift[tid] : 0.f;
        prm[128 + tid] = p.act == VCG_ACT_PRELU ? p.alpha[tid] : (p.act == VCG_ACT_LRELU ? p.act_alpha : 1.f);
    }
    // LDS byte offset of lane (pixel r + dx, half hh)'s fragment of channel group s: boff[dx] ^ (s << 5) -- the swizzle XORs
    // the chunk index 2s + hh with (pos >> 1) & 7, and 2s only touches bits 5-6 of the 128-byte row
    int boff[3];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
        const int pos = r + dx;
        boff[dx] = rg * 8 * V2_ROWB + pos * 128 + ((hh ^ ((pos >> 1) & 7)) << 4);
    }
    const long img_bytes = (long)p.h * p.w_ * 128;

    // one 4-KiB piece (round k of 20) of a tile's halo: slot = 16-byte chunk of the LDS image, in image order.  Issued between MFMAs,
    // so its address arithmetic has to fit an MFMA's shadow: per lane and round the byte offset of the slot's source RELATIVE to the
    // tile's halo origin ((row * w + col) * 128 + chunk * 16) and its halo column are launch constants (20 + 5 registers); a piece is
    // then  offset = tile base + constant,  one column test (left / right image edge)  and a select.  Rows above / below the image
    // need no test: their offsets fall outside the image's buffer descriptor (negative ones wrap to > 4 GiB - 4 MiB); without a
    // next tile the descriptor has zero records and every piece writes zeros into the idle buffer.
    unsigned dma_c[V2_NDMA], dma_colp[(V2_NDMA + 3) / 4];
#pragma unroll
    for (int k = 0; k < V2_NDMA; ++k) {
        const int sl = k * V2_NT + tid, P = sl >> 3, row = P / V2_HC, col = P - row * V2_HC;
        const int cs = (sl & 7) ^ ((col >> 1) & 7);                                // stored chunk (sl & 7) holds source chunk cs
        dma_c[k] = (unsigned)(row * p.w_ + col) * 128u + (unsigned)(cs * 16);
        if ((k & 3) == 0) dma_colp[k >> 2] = 0;
        dma_colp[k >> 2] |= (unsigned)(sl < V2_CHUNKS ? col : 255) << (8 * (k & 3));     // 255: the slots past the tile (round 19, lanes 32-63)
    }
    auto locate = [&](int tile, bool live) {
        const int txi = tile % p.tiles_x, t2 = tile / p.tiles_x, tyi = t2 % p.tiles_y, img = t2 / p.tiles_y;
        const int y0 = tyi * V2_TR - 1, x0 = txi * V2_TC - 1;
        return TileSrc{(unsigned)(y0 * p.w_ + x0) * 128u, x0, make_rsrc((const unsigned char*)p.x + img * img_bytes, (unsigned long)(live ? img_bytes : 0))};
    };
    auto dma = [&](const TileSrc& ts, int buf, int k) {
        if (k == V2_NDMA - 1 && wv != 0) return;                 // wave-uniform
        const int col = (int)((dma_colp[k >> 2] >> (8 * (k & 3))) & 255u);
        unsigned off = ts.base + dma_c[k];
        asm volatile("" : "+v"(off));                            // a select, not a branch around the arithmetic (it would split the schedule)
        off = (unsigned)(ts.x0 + col) < (unsigned)p.w_ ? off : VCG_OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ts.rs, (void __attribute__((address_space(3)))*)(smem + buf * V2_BUF + (k * V2_NT + wv * 64) * 16),
                                                 16, off, 0, 0, 0);
    };

    // the first tile's halo goes out before anything else (it is the HBM round trip every workgroup starts with), the weights behind it
    int tile = blockIdx.x, buf = 0;
    if (tile < p.total) {
        const TileSrc tp = locate(tile, true);
#pragma unroll
        for (int k = 0; k < V2_NDMA; ++k) dma(tp, 0, k);
    }
    // this wave's 36 weight fragments: A[row = co][k = 8hh + j] of (tap, channel group s) = packed [tap][co][ci] chunk 2s + hh
    bf16x8 wa[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) {
        const int tap = i >> 2, s = i & 3;
        wa[i] = __builtin_bit_cast(bf16x8, p.w[(tap * 64 + coh * 32 + r) * 8 + 2 * s + hh]);
    }

    // ---- the pipelined tile loop ---------------------------------------------------------------------------------------
    // A wave's 8 rows are two HALVES of 4 rows with an accumulator set each (2 x 64 registers): while the 144 MFMAs of one half
    // run, the epilogue of the OTHER half (finished 144 MFMAs ago) is issued between them, one 16-byte store unit (8 channels of
    // one row) per k-group -- with one wave per SIMD nothing else could fill the MFMA shadow, and a serial epilogue was 26 % of
    // the tile (profiles/r02_v2_stamps.txt).  Phase A of a tile computes half 0 and drains half 1 of the PREVIOUS tile (whose
    // position is carried in `pv`); phase B computes half 1 and drains half 0.  Per (dx, channel group) a half reads its six halo
    // rows once for the MFMAs of all three dy.
    bf16x8 fb[2][6];
    auto frag = [&](const unsigned char* xb, int h, int g, int b) {
        const int dx = g >> 2, s = g & 3;
#pragma unroll
        for (int j = 0; j < 6; ++j) fb[b][j] = *(const bf16x8*)(xb + (4 * h + j) * V2_ROWB + (boff[dx] ^ (s << 5)));
    };
    auto out_off = [&](const OutPos& o, int n, int q) {
        const int gy = o.gy0 + n;
        unsigned off = (unsigned)(gy * p.w_ + o.gx) * 128u + (unsigned)((coh * 32 + 16 * q + 8 * hh) * 2);
        asm volatile("" : "+v"(off));                            // a select, not a branch around the arithmetic (it would split the schedule)
        return gy < p.h && o.okx ? off : VCG_OOB;
    };
    // one store unit u = (q, n): channels 16q + 8hh + {0..7} of row n.  An MFMA tile leaves lane (pixel, h) with channels
    // 8g+4h+{0..3}; v_permlane32_swap between the register groups (2q, 2q+1) of the two half-waves makes them 8 consecutive ones.
    float sc[8], sh[8], al[8];
    auto epi_params = [&](int q) {
        int prm_o = 0;
        asm volatile("" : "+v"(prm_o));                  // re-read per use: 24 registers not to be held across tiles
        const float* prm_t = prm + prm_o + coh * 32 + 16 * q + 8 * hh;
        if (AFF) {
            *(f32x4*)&sc[0] = *(const f32x4*)(prm_t);
            *(f32x4*)&sc[4] = *(const f32x4*)(prm_t + 4);
            *(f32x4*)&sh[0] = *(const f32x4*)(prm_t + 64);
            *(f32x4*)&sh[4] = *(const f32x4*)(prm_t + 68);
        }
        if (SLOPE) {
            *(f32x4*)&al[0] = *(const f32x4*)(prm_t + 128);
            *(f32x4*)&al[4] = *(const f32x4*)(prm_t + 132);
        }
    };
    // the unit in seven stages, so that a stage fits the shadow of one MFMA (32 cycles = about seven VALU instructions):
    //   0, 1: accumulator reads + permlane swaps of channels 0-3 / 4-7;  2..5: scale / shift / slope of two values each;  6: pack + store
    float ev[8];
    float sacc[32];                                              // STATS: [sum | sum of squares][q][j] of this lane's 16 channels
    unsigned ovb[4];                                             // STATS: the unit's packed output between its store and its two statistics stages
#pragma unroll
    for (int i = 0; i < 32; ++i) sacc[i] = 0.f;
    auto epi_stage = [&](f32x16 (&acc)[4], const OutPos& o, int u, int st) {
        const int q = u >> 2, n = u & 3;
        if (st == 0 && n == 0) epi_params(q);
        if (st < 2) {
#pragma unroll
            for (int j = 2 * st; j < 2 * st + 2; ++j) {
                float lo = acc[n][8 * q + j], hi = acc[n][8 * q + 4 + j];
                swap32(lo, hi);
                ev[j] = lo;
                ev[4 + j] = hi;
            }
            // pin the stage where it is written: LLVM sinks side-effect-free arithmetic across sched_barrier down to its use
            asm volatile("" : "+v"(ev[2 * st]), "+v"(ev[2 * st + 1]), "+v"(ev[2 * st + 4]), "+v"(ev[2 * st + 5]));
        } else if (st < 6) {
#pragma unroll
            for (int j = 2 * (st - 2); j < 2 * (st - 2) + 2; ++j) {
                float t = ev[j];
                if (AFF) t = t * sc[j] + sh[j];
                if (SLOPE) t = t >= 0.f ? t : t * al[j];
                ev[j] = t;
            }
            asm volatile("" : "+v"(ev[2 * (st - 2)]), "+v"(ev[2 * (st - 2) + 1]));
        } else if (st == 6) {
            bf16x8 ov;
#pragma unroll
            for (int j = 0; j < 8; ++j) ov[j] = (__bf16)ev[j];
            // through the image's buffer descriptor: an out-of-image lane (or a half with nothing pending) gets the out-of-range
            // offset instead of an exec mask -- no branch to split the schedule, and hipcc can count the stores in its vmcnt waits
            const u32x4 ob = __builtin_bit_cast(u32x4, ov);
            __builtin_amdgcn_raw_buffer_store_b128(ob, o.rs, (int)out_off(o, n, q), 0, 0);
            if (STATS) {
                // what the statistics stages read: zero for a pixel outside the image (its accumulators hold the bias)
                const unsigned m = (o.gy0 + n < p.h && o.okx) ? 0xFFFFFFFFu : 0u;
#pragma unroll
                for (int d = 0; d < 4; ++d) ovb[d] = ob[d] & m;
                asm volatile("" : "+v"(ovb[0]), "+v"(ovb[1]), "+v"(ovb[2]), "+v"(ovb[3]));
            }
        } else if (STATS) {
            // stages 7, 8: channels 4(st-7) .. 4(st-7)+3 of the unit, unpacked from the stored bf16 pairs
#pragma unroll
            for (int d = 2 * (st - 7); d < 2 * (st - 7) + 2; ++d) {
                const float lo = __uint_as_float(ovb[d] << 16), hi = __uint_as_float(ovb[d] & 0xFFFF0000u);
                sacc[8 * q + 2 * d] += lo;
                sacc[16 + 8 * q + 2 * d] = fmaf(lo, lo, sacc[16 + 8 * q + 2 * d]);
                sacc[8 * q + 2 * d + 1] += hi;
                sacc[16 + 8 * q + 2 * d + 1] = fmaf(hi, hi, sacc[16 + 8 * q + 2 * d + 1]);
            }
            asm volatile("" : "+v"(sacc[8 * q + 4 * (st - 7)]), "+v"(sacc[8 * q + 4 * (st - 7) + 1]), "+v"(sacc[8 * q + 4 * (st - 7) + 2]),
                         "+v"(sacc[8 * q + 4 * (st - 7) + 3]), "+v"(sacc[16 + 8 * q + 4 * (st - 7)]), "+v"(sacc[16 + 8 * q + 4 * (st - 7) + 1]),
                         "+v"(sacc[16 + 8 * q + 4 * (st - 7) + 2]), "+v"(sacc[16 + 8 * q + 4 * (st - 7) + 3]));
        }
    };
    // STATS: the lane sums -> one record: lane (r, hh) ends up with value r = [stat][q][j] summed over the wave's 32 pixels
    auto stats_flush = [&](int unit) {
        const float t = half_wave_reduce_scatter32(sacc, r);
        p.stats[(((long)unit * 2 + rg) * 2 + (r >> 4)) * 64 + coh * 32 + ((r >> 3) & 1) * 16 + 8 * hh + (r & 7)] = t;
#pragma unroll
        for (int i = 0; i < 32; ++i) sacc[i] = 0.f;
    };
    // one phase: 12 k-groups of 12 MFMAs into `acc` (rows 4h..4h+3), the next group's six rows read under them, `drain`'s eight
    // store units in groups 2..9, and (phase A only) two DMA pieces of the next tile in groups 0..9.  The order inside a group is
    // written out and pinned (sched_barrier after every MFMA): left to the scheduler, the drain ends up behind the MFMAs.
    auto phase = [&](f32x16 (&acc)[4], f32x16 (&drain)[4], const OutPos& dpos, const unsigned char* xb, int h, const TileSrc& np, int nbuf,
                     bool has_next) {
        (void)has_next;
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[n][e] = 0.f;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < 12; ++g) {
            const int cur = g & 1, dx = g >> 2, s = g & 3;
            const bool dr = g >= 2 && g < 10, dm = h == 0 && g < 10;
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                const int dy = i >> 2, n = i & 3;
                acc[n] = mfma_bf16(wa[(dy * 3 + dx) * 4 + s], fb[cur][n + dy], acc[n]);
                if (i == 0) {
                    if (g + 1 < 12) frag(xb, h, g + 1, cur ^ 1);
                    else if (h == 0) frag(xb, 1, 0, cur ^ 1);         // phase B's first rows, under phase A's last group
                }
                // unconditional DMA (no branch to split the group): without a next tile its descriptor has no records
                if (i == 1 && dm) dma(np, nbuf, 2 * g);
                if (i == 3 && dm) dma(np, nbuf, 2 * g + 1);
                if (dr && i == 2) epi_stage(drain, dpos, g - 2, 0);
                if (dr && i >= 4 && i <= 9) epi_stage(drain, dpos, g - 2, i - 3);
                if (STATS && dr && i >= 10) epi_stage(drain, dpos, g - 2, i - 3);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    __builtin_amdgcn_s_waitcnt(0x0F70);                          // vmcnt(0): this wave's pieces (and weights) have landed
    lds_barrier();
    unsigned long long st0 = 0, st1 = 0, st2 = 0, st3 = 0, st4 = 0, sum_pa = 0, sum_pb = 0, sum_wt = 0, sum_br = 0;
    (void)st0, (void)st1, (void)st2, (void)st3, (void)st4, (void)sum_pa, (void)sum_pb, (void)sum_wt, (void)sum_br;

    f32x16 acc0[4], acc1[4];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc1[n][e] = 0.f;
    OutPos pv{make_rsrc(p.y, 0), 0, 0, false};                   // nothing pending before the first tile: every offset out of range

    for (; tile < p.total; tile += gridDim.x, buf ^= 1) {
        VCG_STAMP(st0);
        const int next = tile + gridDim.x;
        const bool has_next = next < p.total;
        const TileSrc np = locate(has_next ? next : tile, has_next);
        const unsigned char* xb = smem + buf * V2_BUF;
        const int txi = tile % p.tiles_x, t2 = tile / p.tiles_x, tyi = t2 % p.tiles_y, img = t2 / p.tiles_y;
        const int gx = txi * V2_TC + r;
        const vcg_rsrc yrs = make_rsrc((const unsigned char*)p.y + img * img_bytes, (unsigned long)img_bytes);
        const OutPos p0{yrs, gx, tyi * V2_TR + rg * 8, gx < p.w_}, p1{yrs, gx, tyi * V2_TR + rg * 8 + 4, gx < p.w_};
        frag(xb, 0, 0, 0);
        phase(acc0, acc1, pv, xb, 0, np, buf ^ 1, has_next);      // half 0; drains the previous tile's half 1
        if (STATS && p.stats_per_tile && tile != (int)blockIdx.x) stats_flush(tile - (int)gridDim.x);     // the previous tile is complete
        VCG_STAMP(st1);
        phase(acc1, acc0, p0, xb, 1, np, buf ^ 1, has_next);      // half 1; drains this tile's half 0
        pv = p1;
        VCG_STAMP(st2);
        // The next tile's pieces were issued in phase A: retire them -- vmcnt(8) leaves phase B's eight younger stores in flight
        // (vector memory operations retire in order) -- then the one barrier of the tile: every wave's pieces are in LDS and
        // every wave is done reading this tile's image.
        __builtin_amdgcn_s_waitcnt(0x0F78);
        VCG_STAMP(st3);
        lds_barrier();
        VCG_STAMP(st4);
        VCG_STAMP_ADD(sum_pa, st0, st1);
        VCG_STAMP_ADD(sum_pb, st1, st2);
        VCG_STAMP_ADD(sum_wt, st2, st3);
        VCG_STAMP_ADD(sum_br, st3, st4);
    }
    // the last tile's half 1
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int st = 0; st < (STATS ? 9 : 7); ++st) epi_stage(acc1, pv, u, st);
    if (STATS) stats_flush(p.stats_per_tile ? tile - (int)gridDim.x : (int)blockIdx.x);
#ifdef VCG_STAMPS
    if (lane == 0) {
        unsigned long long* o = vcg_v2_stamp_sums + (blockIdx.x * 4 + wv) * 6;
        o[0] = sum_pa, o[1] = sum_pb, o[2] = sum_wt, o[3] = sum_br;
        o[4] = __builtin_amdgcn_s_memtime() - k_c0, o[5] = __builtin_amdgcn_s_memrealtime() - k_r0;     // whole kernel: core clock / 100 MHz
    }
#endif
}

}  // namespace

extern "C" {

// the v2 kernel finds its halo rows through 32-bit byte offsets against the image's buffer descriptor: the image plus the halo rows
// below it (and a row of slack for the wrapped offsets of the row above it) must stay below 4 GiB, or a halo offset wraps into the image
// bf16_gconv.hip: the 5x5 trunk convolution on the generic kernels, with this file's epilogue contract
int vcg_gconv5x5_c64_bf16_fwd(const vcg_conv_desc* d, const void* x, const void* wfrag, void* y, const vcg_epilogue_bf16* ep, hipStream_t stream);

static bool v2_image_fits(int h, int w) { return ((long)h + V2_HR + 2) * w * 128 + 4096 <= 0xFFFFFFE0l; }

int vcg_conv2d_bf16_stats_records(const vcg_conv_desc* d, int32_t stats_mode) {
    if (d == nullptr) return VCG_E_NULL;
    if (d->n <= 0 || d->h <= 0 || d->w <= 0) return VCG_E_SHAPE;
    if (stats_mode != VCG_STATS_BATCH && stats_mode != VCG_STATS_INSTANCE) return VCG_E_UNSUPPORTED;
    if (!(d->cin == 64 && d->cout == 64 && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad_top == 1 && d->pad_left == 1)) return VCG_E_UNSUPPORTED;
    if (!v2_image_fits(d->h, d->w)) return VCG_E_UNSUPPORTED;
    const long tiles_img = (long)ceil_div(d->w, V2_TC) * ceil_div(d->h, V2_TR), total = tiles_img * d->n;
    if (stats_mode == VCG_STATS_INSTANCE) return (int)(2 * tiles_img);
    return (int)(2 * (total < 256 ? total : 256));
}

int vcg_conv2d_bf16_fwd(const vcg_conv_desc* d, const void* x, const void* w_packed, void* y, const vcg_epilogue_bf16* ep,
                        hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(x);
    VCG_CHECK_PTR(w_packed);
    VCG_CHECK_PTR(y);
    if (d->n <= 0 || d->h <= 0 || d->w <= 0) return VCG_E_SHAPE;
    if (d->oh != d->h || d->ow != d->w) return VCG_E_SHAPE;
    const int act = ep ? ep->act : VCG_ACT_NONE;
    if (act == VCG_ACT_TANH) return VCG_E_UNSUPPORTED;
    if (act == VCG_ACT_PRELU && (!ep || !ep->prelu_alpha)) return VCG_E_NULL;
    if (d->cin == 64 && d->cout == 64 && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad_top == 1 && d->pad_left == 1) {
        C3Params p;
        p.x = (const uint4*)x;
        p.w = (const uint4*)w_packed;
        p.y = (__bf16*)y;
        p.scale = ep ? (const float*)ep->scale : nullptr;
        p.shift = ep ? (const float*)ep->shift : nullptr;
        p.alpha = (ep && act == VCG_ACT_PRELU) ? (const float*)ep->prelu_alpha : nullptr;
        p.res = ep ? (const __bf16*)ep->residual : nullptr;
        p.n = d->n;
        p.h = d->h;
        p.w_ = d->w;
        p.tiles_x = ceil_div(d->w, TC);
        p.tiles_y = ceil_div(d->h, TR);
        p.total = p.n * p.tiles_x * p.tiles_y;
        p.act = act;
        p.act_alpha = ep ? ep->act_alpha : 0.f;
        p.stats = (ep && ep->stats_mode != VCG_STATS_NONE) ? (float*)ep->stats : nullptr;
        p.stats_per_tile = ep && ep->stats_mode == VCG_STATS_INSTANCE;
        if (ep && ep->stats_mode != VCG_STATS_NONE) {
            // statistics come out of the v2 kernel's drain: no activation, no residual input (what stands in front of a normalisation)
            if (!ep->stats) return VCG_E_NULL;
            if (vcg_conv2d_bf16_stats_records(d, ep->stats_mode) <= 0 || act != VCG_ACT_NONE || ep->residual) return VCG_E_UNSUPPORTED;
        }
        const bool aff = p.scale || p.shift, slope = act != VCG_ACT_NONE, res = p.res != nullptr;
        // (the launches below name the instantiations in the order the code object has always held them: v1's eight, then v2's five)
        // v1 where there is a residual input or the image is too large for one buffer descriptor
        if (res || !v2_image_fits(d->h, d->w)) {
            const int grid = p.total < 256 ? p.total : 256;
#define VCG_C3_LAUNCH(A, S, R) do {                                                                                        \
        if (int e = vcg_allow_dyn_lds((const void*)conv3x3_c64_bf16_kernel<A, S, R>, WB + XB + PB)) return e;             \
        conv3x3_c64_bf16_kernel<A, S, R><<<grid, NT, WB + XB + PB, stream>>>(p);                                          \
    } while (0)
            if (!aff) {
                if (!slope) { if (!res) VCG_C3_LAUNCH(false, false, false); else VCG_C3_LAUNCH(false, false, true); }
                else { if (!res) VCG_C3_LAUNCH(false, true, false); else VCG_C3_LAUNCH(false, true, true); }
            } else {
                if (!slope) { if (!res) VCG_C3_LAUNCH(true, false, false); else VCG_C3_LAUNCH(true, false, true); }
                else { if (!res) VCG_C3_LAUNCH(true, true, false); else VCG_C3_LAUNCH(true, true, true); }
            }
#undef VCG_C3_LAUNCH
            VCG_LAUNCH_CHECK();
            return VCG_OK;
        }
        // v2 (one wave per SIMD, weights in registers) everywhere else
        p.tiles_x = ceil_div(d->w, V2_TC);
        p.tiles_y = ceil_div(d->h, V2_TR);
        p.total = p.n * p.tiles_x * p.tiles_y;
        const int grid2 = p.total < 256 ? p.total : 256;
#define VCG_C3V2_LAUNCH(...) do {                                                                                          \
        if (int e = vcg_allow_dyn_lds((const void*)conv3x3_c64_bf16_v2_kernel<__VA_ARGS__>, V2_LDS)) return e;            \
        conv3x3_c64_bf16_v2_kernel<__VA_ARGS__><<<grid2, V2_NT, V2_LDS, stream>>>(p);                                     \
    } while (0)
        if (!p.stats && !aff) {
            if (!slope) VCG_C3V2_LAUNCH(false, false); else VCG_C3V2_LAUNCH(false, true);
        } else if (!p.stats) {
            if (!slope) VCG_C3V2_LAUNCH(true, false); else VCG_C3V2_LAUNCH(true, true);
        } else {
            VCG_C3V2_LAUNCH(true, false, true);          // a null scale / shift reads as 1 / 0
        }
#undef VCG_C3V2_LAUNCH
        VCG_LAUNCH_CHECK();
        return VCG_OK;
    }
    if (d->cin == 64 && d->cout == 64 && d->kh == 5 && d->kw == 5 && d->stride == 1 && d->pad_top == 2 && d->pad_left == 2) {
        // 5x5 trunk of the reference's default generator: the generic kernels' plan (bf16_gconv.hip), w_packed in their fragment layout;
        // no statistics form
        if (ep && ep->stats_mode != VCG_STATS_NONE) return VCG_E_UNSUPPORTED;
        return vcg_gconv5x5_c64_bf16_fwd(d, x, w_packed, y, ep, stream);
    }
    return VCG_E_UNSUPPORTED;
}

}  // extern "C"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// 9x9 stride-1 'same' convolution, 3 -> 64 channels (+bias, PReLU): the generator's initial/conv (model.py:275-276)
// ---------------------------------------------------------------------------------------------------------------
// Input: the fp32 NCHW frames as they arrive; output: bf16 NHWC, i.e. the kernel is also the entry into the bf16
// layout.  In LDS a pixel is RGB0 in bf16 (8 bytes), so 4 consecutive pixels x 4 channels are one 16-wide k-step and
// a lane's operand fragment (2 pixels) is one 8-byte-aligned ds_read2_b64: k-steps = 9 ky x 3 groups of 4 kx (the
// taps kx = 9..11 carry zero weights) = 27, against 36 of the 64-channel 3x3 convolution.  Same skeleton as
// conv3x3_c64_bf16_kernel: 6 compute + 2 loader waves, weights (54 KiB of operand fragments) resident in LDS,
// 12x32-pixel tiles, permlane-swapped 16-byte stores.  The kernel is bound by its 128 bytes of output per pixel.
// The same kernel serves every convolution ON THREE INPUT CHANNELS (template <KH, NG, S>: KH kernel rows, NG groups of 4 kernel columns,
// stride S): 9x9 stride 1 above (KH 9, NG 3), the critics' first layers -- 4x4 stride 2 (PatchGAN block 1: KH 4, NG 1, S 2) and 3x3 stride 1
// (simple_512 / thin_512 block 1, model.py:839: KH 3, NG 1) -- with bias + LeakyReLU / PReLU in the epilogue.  An output tile of 12x32
// pixels reads a halo of (12 S + KH - S) x (31 S + 4 NG + 1) input pixels; lane r's fragment sits at column r S + 4 j + 2 hh.
// NSRC (the input-driven gates below): the input is NSRC stacked 3-channel sources, fp32 NCHW [n][3 NSRC][h][w]; each source has a halo tile
// of its own in LDS (XB1 bytes apart) and its own KH x NG k-steps -- the convolution is linear in its input channels.
template <int KH, int NG, int S, int NSRC = 1>
struct I3Cfg {
    static constexpr int HR = TR * S + KH - S;                    // halo rows           (9x9: 20)
    static constexpr int HC = (31 * S + 4 * NG + 2) & ~1;         // halo columns, even  (9x9: 44)
    static constexpr int ROWB = HC * 8;
    static constexpr int XB1 = (HR * ROWB + 15) & ~15;            // one source's halo tile (9x9: 7040 B)
    static constexpr int XB = NSRC * XB1;
    static constexpr int NK = NSRC * KH * NG;                     // k-steps of 16
    static constexpr int WB = NK * 64 * 32;                       // 9x9: 55296 B: [k-step][out-channel][half][8 bf16]
    static constexpr int NPIX = HR * HC;                          // 9x9: 880 pixels per halo tile
    static constexpr int NPRE = (NPIX + NLW * 64 - 1) / (NLW * 64);       // pixels per loader lane (9x9: 7)
    static constexpr int LDS = WB + XB + 512;
};

struct I9Params {
    const float* x;          // fp32 NCHW [n][3][h][w]
    const uint4* w;          // packed fragments (vcg_pack_first9x9_bf16)
    const float* bias;       // [cout] or null
    union {
        const float* alpha;  // PReLU slopes [cout] or null (none)
        const __bf16* dy;    // GATE_BWD: the gradient at the gate's output, bf16 NHWC [n][h][w][cout]
    };
    __bf16* y;               // bf16 NHWC [n][h][w][cout]
    __bf16* z;               // optional bf16 NHWC [n][h][w][cout]: the value in front of the PReLU (its backward needs the sign and, for the slope gradient, the value);
                             // GATE_BWD: da, the gradient in front of the gate convolution's bias (y is dm)
    const __bf16* mask;      // optional bf16 NHWC [n][h][w][cout]: y *= (mask > 0 ? 1 : mask_slope)  (data gradient in front of a LeakyReLU);
                             // GATE instantiations: the gated tensor m, y = sigmoid(conv + bias) * m
    float mask_slope;
    union {
        float* chsum;        // optional [workgroups per channel block * 6][cout]: per-wave sums of the stored output per channel (a bias gradient)
        const __bf16* dres;  // GATE_BWD: optional bf16 NHWC gradient joining at m, added to dm in fp32 before the one rounding
    };
    int n, h, w_, cout, tiles_x, tiles_y, total;        // cout = 64 * nblk; workgroup b serves channel block b % nblk; h, w_: INPUT size
    int oh, ow, pad_top, pad_left;                      // output size and the 'before' pads (9x9 'same': h, w_, 4, 4)
    float slope;                                        // without alpha: LeakyReLU slope (1 = no activation)
    int xcd_group;                                      // block_and_stream
};

// Diagnostic build only (-DVCG_STAMPS, scripts/micro/stamps.py): s_memtime sums per wave [MFMA loop, barrier after it, epilogue, barrier
// after it, tiles, kernel clocks] (compute waves) / [fetch issue, barrier 1, stash, barrier 2, tiles, kernel clocks] (loader waves)
VCG_STAMP_SUMS(i9, 512 * 8 * 6);

// sigmoid from one v_exp_f32 and one v_rcp_f32 (as fast_tanh, bf16_conv9x9_to3.hip): 1 / (1 + exp(-x)).  exp(-x) carries the rounding of x log2(e) and the
// 1-ulp v_exp_f32, a relative error below 2^-24 (2 + 1.5 |x|); the sigmoid's absolute error is s (1 - s) times that, <= 3e-7 for every x
// (s (1 - s) |x| <= 0.23) -- four orders below the bf16 rounding of the product it feeds (up to 2^-8 relative).  Saturates cleanly: exp -> inf
// gives rcp(inf) = 0, exp -> 0 gives 1.
__device__ __forceinline__ float fast_sigmoid(float x) { return __frcp_rn(1.f + __expf(-x)); }

// the same sigmoid (bit for bit) and its slope s (1 - s) = e / (1 + e)^2 with e = exp(-x), formed from e and not as s * (1 - s): at large x the
// fp32 rounding of s next to 1 leaves 1 - s few significant bits (3e-8 absolute of 6e-6 at x = 12 is 2^-8 relative, a whole bf16 rounding).
// e * s * s is good to a few fp32 ulp for every x; the clamp keeps e = inf (x < -88, s = 0) from making inf * 0.
__device__ __forceinline__ float fast_sigmoid_slope(float x, float& s) {
    const float e = __expf(-x);
    s = __frcp_rn(1.f + e);
    return fminf(e, 0x1p+60f) * s * s;
}

// the epilogue forms of conv_c3to64_bf16_kernel
constexpr int GATE_NONE = 0;     // bias + PReLU / LeakyReLU [* mask]
constexpr int GATE_FWD = 1;      // y = bf16(sigmoid(conv + bias) * m)
constexpr int GATE_BWD = 2;      // s = sigmoid(conv + bias) recomputed;  dm = bf16(dy * s + dres),  da = bf16(dy * m * s * (1 - s))

// GATE (input-driven attention gates of make_upscaler_attention, model.py:33-36, 86-90): the epilogue is y = bf16(sigmoid(conv + bias) * m)
// with m (p.mask) a bf16 NHWC tensor of the output's shape, requested under the MFMA loop like the LeakyReLU mask; the attention tensor
// itself never leaves the registers.  GATE_BWD is that gate's backward in the same launch shape: the MFMA loop recomputes the pre-activation
// from the frames, dy and the joining gradient dres are requested next to m, and the epilogue writes dm (p.y) and da (p.z) -- in training
// the attention tensor does not reach HBM either.
template <int KH, int NG, int S, int NSRC = 1, int GATE = GATE_NONE>
__global__ __launch_bounds__(NT, 1) void conv_c3to64_bf16_kernel(I9Params p) {
    using C = I3Cfg<KH, NG, S, NSRC>;
    constexpr int I_HC = C::HC, I_ROWB = C::ROWB, I_XB = C::XB, I_XB1 = C::XB1, I_WB = C::WB, I_NPIX = C::NPIX, I_NPRE = C::NPRE, NK = C::NK;
#ifdef VCG_STAMPS
    unsigned long long s0 = 0, s1 = 0, s2 = 0, s3 = 0, ntl = 0, st0, st1, st2, st3, st4;
    const unsigned long long k_c0 = __builtin_amdgcn_s_memtime();
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* wl = smem;
    unsigned char* xl = smem + I_WB;
    float* prm = (float*)(smem + I_WB + I_XB);       // bias[64], slope[64]
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nblk = p.cout >> 6, nwg = gridDim.x / nblk;
    int cb, wg0;
    block_and_stream(nblk, p.xcd_group, cb, wg0);

    for (int c = tid; c < I_WB / 16; c += NT) ((uint4*)wl)[c] = p.w[(long)cb * (I_WB / 16) + c];
    if (tid < 64) {
        prm[tid] = p.bias ? p.bias[cb * 64 + tid] : 0.f;
        if constexpr (GATE == GATE_BWD) prm[64 + tid] = 1.f;      // (the alpha slot holds dy)
        else prm[64 + tid] = p.alpha ? p.alpha[cb * 64 + tid] : p.slope;
    }
    const long plane = (long)p.h * p.w_;

    if (wv >= NCW) {
        const int lt = tid - NCW * 64;
        float pre[NSRC][I_NPRE][3];
        auto fetch = [&](int tile) {
            const int txi = tile % p.tiles_x, t2 = tile / p.tiles_x, tyi = t2 % p.tiles_y, img = t2 / p.tiles_y;
            const int y0 = tyi * TR * S - p.pad_top, x0 = txi * TC * S - p.pad_left;
            const float* xi = p.x + (long)img * (3 * NSRC) * plane;
#pragma unroll
            for (int i = 0; i < I_NPRE; ++i) {
                const int pix = min(lt + NLW * 64 * i, I_NPIX - 1);
                const int row = pix / I_HC, col = pix - row * I_HC;
                const int gy = y0 + row, gx = x0 + col;
                const bool ok = (unsigned)gy < (unsigned)p.h && (unsigned)gx < (unsigned)p.w_;
                const long o = (long)min(max(gy, 0), p.h - 1) * p.w_ + min(max(gx, 0), p.w_ - 1);
#pragma unroll
                for (int sc = 0; sc < NSRC; ++sc)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float v = xi[(sc * 3 + ch) * plane + o];
                        pre[sc][i][ch] = ok ? v : 0.f;
                    }
            }
        };
        auto stash = [&]() {
#pragma unroll
            for (int sc = 0; sc < NSRC; ++sc)
#pragma unroll
                for (int i = 0; i < I_NPRE; ++i) {
                    const int pix = min(lt + NLW * 64 * i, I_NPIX - 1);
                    bf16x4 v;
                    v[0] = (__bf16)pre[sc][i][0];
                    v[1] = (__bf16)pre[sc][i][1];
                    v[2] = (__bf16)pre[sc][i][2];
                    v[3] = (__bf16)0.f;
                    *(bf16x4*)(xl + sc * I_XB1 + pix * 8) = v;
                }
        };
        int tile = wg0;
        if (tile < p.total) fetch(tile);
        stash();
        lds_barrier();
        for (; tile < p.total; tile += nwg) {
            const int next = tile + nwg;
            VCG_STAMP(st0);
            if (next < p.total) fetch(next);
            VCG_STAMP(st1);
            lds_barrier();
            VCG_STAMP(st2);
            if (next < p.total) stash();
            VCG_STAMP(st3);
            lds_barrier();
            VCG_STAMP(st4);
            VCG_STAMP_ADD(s0, st0, st1); VCG_STAMP_ADD(s1, st1, st2); VCG_STAMP_ADD(s2, st2, st3); VCG_STAMP_ADD(s3, st3, st4);
#ifdef VCG_STAMPS
            ++ntl;
#endif
        }
#ifdef VCG_STAMPS
        if (lane == 0 && blockIdx.x < 512) {
            unsigned long long* o = vcg_i9_stamp_sums + (blockIdx.x * 8 + wv) * 6;
            o[0] = s0, o[1] = s1, o[2] = s2, o[3] = s3, o[4] = ntl, o[5] = __builtin_amdgcn_s_memtime() - k_c0;
        }
#endif
        return;
    }

    const int aoff = r * 32 + hh * 16;                         // weight fragment of (co = r [+32], half)
    const unsigned char* xb = xl + (wv * 2 * S) * I_ROWB + (r * S + 2 * hh) * 8;
    float csum[32];                                            // p.chsum: this lane's 32 channels [mt][q][j], summed over its pixels
#pragma unroll
    for (int i = 0; i < 32; ++i) csum[i] = 0.f;
    lds_barrier();

    for (int tile = wg0; tile < p.total; tile += nwg) {
        const int txi = tile % p.tiles_x, t2 = tile / p.tiles_x, tyi = t2 % p.tiles_y, img = t2 / p.tiles_y;
        const int gx = txi * TC + r, gy0 = tyi * TR + wv * 2;
        const bool okx = gx < p.ow;

        // the LeakyReLU mask of this wave's 2 x 32 pixels (data gradient in front of an activation): requested here, read in the epilogue --
        // under the MFMA loop.  (Loaded where it was used, each of the eight 16-byte loads waited out an HBM round trip: 6.6k of a tile's
        // 21k cycles, profiles/r03_i9_stamps.txt.)
        bf16x8 mk[2][2][2];
        bf16x8 gd[2][2][2], gr[2][2][2];                       // GATE_BWD: dy and dres of the same pixels
        if (GATE != GATE_NONE || p.mask) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int pt = 0; pt < 2; ++pt) {
                        const int gy = gy0 + pt;
                        const long o = ((long)(img * p.oh + min(gy, p.oh - 1)) * p.ow + min(gx, p.ow - 1)) * p.cout + cb * 64 + mt * 32 + 16 * q + 8 * hh;
                        mk[mt][q][pt] = *(const bf16x8*)(p.mask + o);
                        if constexpr (GATE == GATE_BWD) {
                            gd[mt][q][pt] = *(const bf16x8*)(p.dy + o);
                            // without a joining gradient the sum below still adds a zero: the same bits as a dres of zeros
#pragma unroll
                            for (int j = 0; j < 8; ++j) gr[mt][q][pt][j] = (__bf16)0.f;
                            if (p.dres) gr[mt][q][pt] = *(const bf16x8*)(p.dres + o);
                        }
                    }
        }

        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

        bf16x8 fa[2][2], fb[2][2];
        auto frag = [&](auto ic) {
            constexpr int i = decltype(ic)::value, sc = i / (KH * NG), i1 = i - sc * (KH * NG), ky = i1 / NG, j = i1 - NG * ky, buf = i & 1;
            const unsigned char* wa = wl + i * 2048 + aoff;
            fa[buf][0] = *(const bf16x8*)(wa);
            fa[buf][1] = *(const bf16x8*)(wa + 1024);
            const unsigned char* b0 = xb + sc * I_XB1 + ky * I_ROWB + j * 32;
            bf16x4 lo = *(const bf16x4*)(b0), hi = *(const bf16x4*)(b0 + 8);
            fb[buf][0] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            lo = *(const bf16x4*)(b0 + S * I_ROWB);
            hi = *(const bf16x4*)(b0 + S * I_ROWB + 8);
            fb[buf][1] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        };
        VCG_STAMP(st0);
        frag(std::integral_constant<int, 0>{});
        static_for<NK>([&](auto ic) {
            constexpr int i = decltype(ic)::value, cur = i & 1;
            if constexpr (i + 1 < NK) frag(std::integral_constant<int, i + 1>{});
            __builtin_amdgcn_sched_barrier(0);
            acc[0][0] = mfma_bf16(fa[cur][0], fb[cur][0], acc[0][0]);
            acc[0][1] = mfma_bf16(fa[cur][0], fb[cur][1], acc[0][1]);
            acc[1][0] = mfma_bf16(fa[cur][1], fb[cur][0], acc[1][0]);
            acc[1][1] = mfma_bf16(fa[cur][1], fb[cur][1], acc[1][1]);
            __builtin_amdgcn_sched_barrier(0);
        });
        VCG_STAMP(st1);
        lds_barrier();
        VCG_STAMP(st2);

#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int co = mt * 32 + 16 * q + 8 * hh;
                float sh[8], al[8];
                *(f32x4*)&sh[0] = *(const f32x4*)(prm + co);
                *(f32x4*)&sh[4] = *(const f32x4*)(prm + co + 4);
                *(f32x4*)&al[0] = *(const f32x4*)(prm + 64 + co);
                *(f32x4*)&al[4] = *(const f32x4*)(prm + 64 + co + 4);
#pragma unroll
                for (int pt = 0; pt < 2; ++pt) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float lo = acc[mt][pt][8 * q + j], hi = acc[mt][pt][8 * q + 4 + j];
                        swap32(lo, hi);
                        v[j] = lo;
                        v[4 + j] = hi;
                    }
                    const int gy = gy0 + pt;
                    const bool ok = gy < p.oh && okx;
                    const long o = ((long)(img * p.oh + min(gy, p.oh - 1)) * p.ow + min(gx, p.ow - 1)) * p.cout + cb * 64 + co;
                    bf16x8 ov, zv;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float u = v[j] + sh[j];
                        zv[j] = (__bf16)u;
                        if constexpr (GATE == GATE_BWD) {
                            float s;
                            const float slope = fast_sigmoid_slope(u, s), g = (float)gd[mt][q][pt][j];
                            zv[j] = (__bf16)(g * (float)mk[mt][q][pt][j] * slope);                   // da
                            u = g * s + (float)gr[mt][q][pt][j];                                     // dm: fp32 sum, rounded once
                        } else if constexpr (GATE == GATE_FWD) {
                            u = fast_sigmoid(u) * (float)mk[mt][q][pt][j];           // fp32 product, rounded once
                        } else {
                            u = u >= 0.f ? u : u * al[j];
                            if (p.mask) u = (float)mk[mt][q][pt][j] > 0.f ? u : u * p.mask_slope;
                        }
                        ov[j] = (__bf16)u;
                    }
                    if (ok) *(bf16x8*)(p.y + o) = ov;
                    if (GATE == GATE_BWD && ok) *(bf16x8*)(p.z + o) = zv;
                    if (GATE == GATE_NONE && p.z && ok) *(bf16x8*)(p.z + o) = zv;
                    if (GATE == GATE_NONE && p.chsum && ok) {                             // the values as stored
#pragma unroll
                        for (int j = 0; j < 8; ++j) csum[mt * 16 + q * 8 + j] += (float)ov[j];
                    }
                }
            }
        VCG_STAMP(st3);
        lds_barrier();
        VCG_STAMP(st4);
        VCG_STAMP_ADD(s0, st0, st1); VCG_STAMP_ADD(s1, st1, st2); VCG_STAMP_ADD(s2, st2, st3); VCG_STAMP_ADD(s3, st3, st4);
#ifdef VCG_STAMPS
        ++ntl;
#endif
    }
#ifdef VCG_STAMPS
    if (lane == 0 && blockIdx.x < 512) {
        unsigned long long* o = vcg_i9_stamp_sums + (blockIdx.x * 8 + wv) * 6;
        o[0] = s0, o[1] = s1, o[2] = s2, o[3] = s3, o[4] = ntl, o[5] = __builtin_amdgcn_s_memtime() - k_c0;
    }
#endif
    if (GATE == GATE_NONE && p.chsum) {
        // lane (r, hh) ends up with the sum of value r = [mt][q][j] over the wave's 32 pixel lanes: channel mt*32 + 16q + 8hh + j
        const float t = half_wave_reduce_scatter32(csum, r);
        p.chsum[(long)(wg0 * NCW + wv) * p.cout + cb * 64 + (r >> 4) * 32 + ((r >> 3) & 1) * 16 + 8 * hh + (r & 7)] = t;
    }
}

__global__ void pack_first9x9_kernel(const float* __restrict__ w, uint4* __restrict__ out, int cout, int dgrad, int kh, int kw, int ng) {
    // out[channel block][k-step = ky*ng+j][co in block][half] = 8 bf16: (kx = 4j+2*half, RGB0), (kx+1, RGB0)
    //   dgrad == 0: w is Keras (kh,kw,3,cout), the forward kernel of a 3 -> cout convolution
    //   dgrad == 1: w is Keras (kh,kw,cout,3), the kernel of a cout -> 3 convolution; packed for its DATA GRADIENT
    //               (a 3 -> cout convolution with the taps flipped):  W'[ky][kx][c][m] = w[kh-1-ky][kw-1-kx][m][c]
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int nk = kh * ng;
    if (idx >= (cout >> 6) * nk * 64 * 2) return;
    const int h = idx & 1, co = (idx >> 1) & 63, ks = (idx >> 7) % nk, cb = idx / (nk * 128), ky = ks / ng, j = ks - ng * ky;
    const int m = cb * 64 + co;
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int kx = 4 * j + 2 * h + (e >> 2), c = e & 3;
        float x = 0.f;
        if (kx < kw && c < 3) x = dgrad ? w[(((kh - 1 - ky) * kw + (kw - 1 - kx)) * cout + m) * 3 + c] : w[((ky * kw + kx) * 3 + c) * cout + m];
        v[e] = (__bf16)x;
    }
    out[idx] = __builtin_bit_cast(uint4, v);
}

__global__ void pack_in_gate_kernel(const float* __restrict__ w, uint4* __restrict__ out, int cin, int cout, int kh, int kw, int ng) {
    // w: Keras (kh,kw,cin,cout), cin = 3 nsrc -> out[channel block][k-step = (src*kh + ky)*ng + j][co in block][half] = 8 bf16:
    // (kx = 4j+2*half, RGB0 of source src), (kx+1, RGB0 of source src); kernel columns past kw carry zeros
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int nk = (cin / 3) * kh * ng;
    if (idx >= (cout >> 6) * nk * 64 * 2) return;
    const int h = idx & 1, co = (idx >> 1) & 63, ks = (idx >> 7) % nk, cb = idx / (nk * 128);
    const int src = ks / (kh * ng), k1 = ks - src * kh * ng, ky = k1 / ng, j = k1 - ng * ky;
    const int m = cb * 64 + co;
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int kx = 4 * j + 2 * h + (e >> 2), c = e & 3;
        float x = 0.f;
        if (kx < kw && c < 3) x = w[((ky * kw + kx) * cin + src * 3 + c) * cout + m];
        v[e] = (__bf16)x;
    }
    out[idx] = __builtin_bit_cast(uint4, v);
}

}  // namespace

template <int KH, int NG, int S, int NSRC = 1, int GATE = GATE_NONE>
static int launch_conv3ch(I9Params p, hipStream_t stream) {
    using C = I3Cfg<KH, NG, S, NSRC>;
    if (int e = vcg_allow_dyn_lds((const void*)conv_c3to64_bf16_kernel<KH, NG, S, NSRC, GATE>, C::LDS)) return e;
    const int nblk = p.cout / 64;
    int per = 1024 / nblk;
    if (per > p.total) per = p.total;
    conv_c3to64_bf16_kernel<KH, NG, S, NSRC, GATE><<<per * nblk, NT, C::LDS, stream>>>(p);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

extern "C" {

int vcg_pack_first9x9_bf16(const void* w, void* out, hipStream_t stream) {
    return vcg_pack_conv9x9_3ch_bf16(w, 64, 0, out, stream);
}

int vcg_pack_conv9x9_3ch_bf16(const void* w, int32_t cout, int32_t dgrad, void* out, hipStream_t stream) {
    VCG_CHECK_PTR(w);
    VCG_CHECK_PTR(out);
    if (cout <= 0 || cout % 64 != 0) return VCG_E_SHAPE;
    const int total = (cout >> 6) * 27 * 64 * 2;
    pack_first9x9_kernel<<<(total + 255) / 256, 256, 0, stream>>>((const float*)w, (uint4*)out, cout, dgrad, 9, 9, 3);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

// Conv2D(cout, k, strides s) on 3 input channels, fp32 NCHW frames -> bf16 NHWC (+bias, LeakyReLU): the critics' block 1
// (model.py:839 3x3 stride 1; PatchGAN 4x4 stride 2).  wfrag: vcg_conv3ch_bf16_wfrag_bytes(kh, cout) bytes from vcg_pack_conv3ch_bf16.
static bool conv3ch_supported(int kh, int kw, int stride) { return (kh == 4 && kw == 4 && stride == 2) || (kh == 3 && kw == 3 && stride == 1); }

size_t vcg_conv3ch_bf16_wfrag_bytes(int32_t kh, int32_t kw, int32_t cout) {
    if (kh <= 0 || kw <= 0 || kw > 4 || cout <= 0 || cout % 64) return 0;
    return (size_t)(cout >> 6) * kh * 64 * 2 * 16;
}

int vcg_pack_conv3ch_bf16(const void* w, int32_t kh, int32_t kw, int32_t cout, void* out, hipStream_t stream) {
    VCG_CHECK_PTR(w);
    VCG_CHECK_PTR(out);
    if (cout <= 0 || cout % 64 != 0 || kh <= 0 || kw <= 0) return VCG_E_SHAPE;
    if (kw > 4) return VCG_E_UNSUPPORTED;
    const int total = (cout >> 6) * kh * 64 * 2;
    pack_first9x9_kernel<<<(total + 255) / 256, 256, 0, stream>>>((const float*)w, (uint4*)out, cout, 0, kh, kw, 1);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

static int conv9x9_3ch_wgs(const vcg_conv_desc* d, int cout) {          // workgroups per output-channel block
    const int nblk = cout / 64;
    const long total = (long)d->n * ceil_div(d->w, TC) * ceil_div(d->h, TR);
    const int per = 512 / nblk;                                   // 62 KiB of LDS: two workgroups per CU
    return (int)(per > total ? total : per);
}

static int launch_conv9x9_3ch(const vcg_conv_desc* d, int cout, const void* x, const void* wfrag, const void* bias, const void* prelu_alpha,
                              const void* mask, float mask_slope, void* y, float* chsum, hipStream_t stream, void* z = nullptr) {
    const int nblk = cout / 64;
    if (cout % 64 != 0 || nblk < 1 || nblk > 8 || (nblk & (nblk - 1))) return VCG_E_UNSUPPORTED;
    I9Params p;
    p.chsum = chsum;
    p.x = (const float*)x;
    p.w = (const uint4*)wfrag;
    p.bias = (const float*)bias;
    p.alpha = (const float*)prelu_alpha;
    p.y = (__bf16*)y;
    p.z = (__bf16*)z;
    p.mask = (const __bf16*)mask;
    p.mask_slope = mask_slope;
    p.n = d->n;
    p.h = d->h;
    p.w_ = d->w;
    p.cout = cout;
    p.tiles_x = ceil_div(d->w, TC);
    p.tiles_y = ceil_div(d->h, TR);
    p.total = p.n * p.tiles_x * p.tiles_y;
    p.oh = d->h; p.ow = d->w; p.pad_top = 4; p.pad_left = 4; p.slope = 1.f;
    p.xcd_group = 0;      // always the plain mapping; dropping the parameter changes device code and waits for a change that measures
    using C = I3Cfg<9, 3, 1>;
    if (int e = vcg_allow_dyn_lds((const void*)conv_c3to64_bf16_kernel<9, 3, 1>, C::LDS)) return e;
    const int per = conv9x9_3ch_wgs(d, cout);
    conv_c3to64_bf16_kernel<9, 3, 1><<<per * nblk, NT, C::LDS, stream>>>(p);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

int vcg_conv3ch_bf16_fwd(const vcg_conv_desc* d, const void* x, const void* wfrag, const void* bias, float lrelu_slope, void* y, hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(x);
    VCG_CHECK_PTR(wfrag);
    VCG_CHECK_PTR(y);
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->oh <= 0 || d->ow <= 0 || d->pad_top < 0 || d->pad_left < 0) return VCG_E_SHAPE;
    if (d->cin != 3 || !conv3ch_supported(d->kh, d->kw, d->stride)) return VCG_E_UNSUPPORTED;
    const int nblk = d->cout / 64;
    if (d->cout % 64 != 0 || nblk < 1 || nblk > 8 || (nblk & (nblk - 1))) return VCG_E_UNSUPPORTED;
    I9Params p;
    p.chsum = nullptr;
    p.x = (const float*)x;
    p.w = (const uint4*)wfrag;
    p.bias = (const float*)bias;
    p.alpha = nullptr;
    p.xcd_group = 0;      // always the plain mapping; dropping the parameter changes device code and waits for a change that measures
    p.slope = lrelu_slope;
    p.y = (__bf16*)y;
    p.z = nullptr;
    p.mask = nullptr;
    p.mask_slope = 0.f;
    p.n = d->n; p.h = d->h; p.w_ = d->w; p.cout = d->cout;
    p.oh = d->oh; p.ow = d->ow; p.pad_top = d->pad_top; p.pad_left = d->pad_left;
    p.tiles_x = ceil_div(d->ow, TC);
    p.tiles_y = ceil_div(d->oh, TR);
    p.total = p.n * p.tiles_x * p.tiles_y;
    if (d->kh == 4) return launch_conv3ch<4, 1, 2>(p, stream);
    return launch_conv3ch<3, 1, 1>(p, stream);
}

// Input-driven sigmoid gate (residual_block_attention model.py:33-36, upsampling_block_attention :80-90): y = sigmoid(conv_kxk(u) + bias) * m
static bool in_gate_supported(int cin, int kh, int kw, int cout) {
    const int nblk = cout / 64;
    return (cin == 3 || cin == 6) && kh == kw && (kh == 3 || kh == 5) && cout > 0 && cout % 64 == 0 && nblk <= 8 && !(nblk & (nblk - 1));
}

size_t vcg_conv_in_gate_bf16_wfrag_bytes(int32_t cin, int32_t kh, int32_t kw, int32_t cout) {
    if (!in_gate_supported(cin, kh, kw, cout)) return 0;
    return (size_t)(cout >> 6) * (cin / 3) * kh * ceil_div(kw, 4) * 64 * 2 * 16;
}

int vcg_pack_conv_in_gate_bf16(const void* w_hwio, int32_t cin, int32_t kh, int32_t kw, int32_t cout, void* out, hipStream_t stream) {
    VCG_CHECK_PTR(w_hwio);
    VCG_CHECK_PTR(out);
    if (!in_gate_supported(cin, kh, kw, cout)) return VCG_E_UNSUPPORTED;
    const int ng = ceil_div(kw, 4), total = (cout >> 6) * (cin / 3) * kh * ng * 64 * 2;
    pack_in_gate_kernel<<<(total + 255) / 256, 256, 0, stream>>>((const float*)w_hwio, (uint4*)out, cin, cout, kh, kw, ng);
    VCG_LAUNCH_CHECK();
    return VCG_OK;
}

int vcg_conv_in_gate_bf16_fwd(const vcg_conv_desc* d, const void* u, const void* wfrag, const void* bias, const void* m, void* y, hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(u);
    VCG_CHECK_PTR(wfrag);
    VCG_CHECK_PTR(m);
    VCG_CHECK_PTR(y);
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->oh != d->h || d->ow != d->w) return VCG_E_SHAPE;
    if (!in_gate_supported(d->cin, d->kh, d->kw, d->cout) || d->stride != 1 || d->pad_top != d->kh / 2 || d->pad_left != d->kw / 2)
        return VCG_E_UNSUPPORTED;
    if (y == m) return VCG_E_UNSUPPORTED;                 // the residual block still adds the ungated m
    if ((long)d->n * ceil_div(d->w, TC) * ceil_div(d->h, TR) > 0x7FFFFFFFl) return VCG_E_UNSUPPORTED;
    I9Params p;
    p.chsum = nullptr;
    p.x = (const float*)u;
    p.w = (const uint4*)wfrag;
    p.bias = (const float*)bias;
    p.alpha = nullptr;
    p.xcd_group = 0;
    p.slope = 1.f;
    p.y = (__bf16*)y;
    p.z = nullptr;
    p.mask = (const __bf16*)m;
    p.mask_slope = 0.f;
    p.n = d->n; p.h = d->h; p.w_ = d->w; p.cout = d->cout;
    p.oh = d->oh; p.ow = d->ow; p.pad_top = d->pad_top; p.pad_left = d->pad_left;
    p.tiles_x = ceil_div(d->ow, TC);
    p.tiles_y = ceil_div(d->oh, TR);
    p.total = p.n * p.tiles_x * p.tiles_y;
    if (d->kh == 3) return d->cin == 3 ? launch_conv3ch<3, 1, 1, 1, GATE_FWD>(p, stream) : launch_conv3ch<3, 1, 1, 2, GATE_FWD>(p, stream);
    return d->cin == 3 ? launch_conv3ch<5, 2, 1, 1, GATE_FWD>(p, stream) : launch_conv3ch<5, 2, 1, 2, GATE_FWD>(p, stream);
}

// The gate's backward (model.py:33-36 differentiated): s = sigmoid(conv_kxk(u) + bias) is recomputed from the frames,
//   dm = bf16(dy * s + dres)        (dres: a gradient joining at m, or NULL; fp32 sum, one rounding -- vcg_conv2d_nhwc_bf16_dgrad_add's rule)
//   da = bf16(dy * m * s * (1 - s)) (the gradient in front of the gate convolution's bias: vcg_conv3ch_bf16_wgrad's dz)
// in one launch, no workspace.  Served: cin 3, 3x3 / 5x5, stride 1, cout 64 (the residual blocks' gates); up: cin 6, cout 64 or 128.
static int gate_bwd(const vcg_conv_desc* d, bool up, const void* u, const void* wfrag, const void* bias, const void* m, const void* dy,
                    const void* dres, void* dm, void* da, hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(u);
    VCG_CHECK_PTR(wfrag);
    VCG_CHECK_PTR(m);
    VCG_CHECK_PTR(dy);
    VCG_CHECK_PTR(dm);
    VCG_CHECK_PTR(da);
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->oh != d->h || d->ow != d->w) return VCG_E_SHAPE;
    const bool served = up ? d->cin == 6 && (d->cout == 64 || d->cout == 128) : d->cin == 3 && d->cout == 64;
    if (!served || d->kh != d->kw || (d->kh != 3 && d->kh != 5) || d->stride != 1 || d->pad_top != d->kh / 2 || d->pad_left != d->kw / 2)
        return VCG_E_UNSUPPORTED;
    if (dm == dres || dm == m || dm == da) return VCG_E_UNSUPPORTED;          // m still feeds the block's Add; dres may be another branch's gradient
    if ((long)d->n * ceil_div(d->w, TC) * ceil_div(d->h, TR) > 0x7FFFFFFFl) return VCG_E_UNSUPPORTED;
    I9Params p;
    p.dres = (const __bf16*)dres;
    p.x = (const float*)u;
    p.w = (const uint4*)wfrag;
    p.bias = (const float*)bias;
    p.dy = (const __bf16*)dy;
    p.xcd_group = 0;
    p.slope = 1.f;
    p.y = (__bf16*)dm;
    p.z = (__bf16*)da;
    p.mask = (const __bf16*)m;
    p.mask_slope = 0.f;
    p.n = d->n; p.h = d->h; p.w_ = d->w; p.cout = d->cout;
    p.oh = d->oh; p.ow = d->ow; p.pad_top = d->pad_top; p.pad_left = d->pad_left;
    p.tiles_x = ceil_div(d->ow, TC);
    p.tiles_y = ceil_div(d->oh, TR);
    p.total = p.n * p.tiles_x * p.tiles_y;
    if (d->kh == 3) return up ? launch_conv3ch<3, 1, 1, 2, GATE_BWD>(p, stream) : launch_conv3ch<3, 1, 1, 1, GATE_BWD>(p, stream);
    return up ? launch_conv3ch<5, 2, 1, 2, GATE_BWD>(p, stream) : launch_conv3ch<5, 2, 1, 1, GATE_BWD>(p, stream);
}

int vcg_conv_in_gate_bf16_bwd(const vcg_conv_desc* d, const void* u, const void* wfrag, const void* bias, const void* m, const void* dy,
                              const void* dres, void* dm, void* da, hipStream_t stream) {
    return gate_bwd(d, false, u, wfrag, bias, m, dy, dres, dm, da, stream);
}

// The same backward for the gates of upsampling_block_attention (model.py:80-90 differentiated): u is the 6-channel Concatenate of the two
// resized frames -- NSRC = 2, the stacked halo tiles of the forward -- and cout is the up-sampling stage's 64 or 128.
int vcg_conv_in_gate_up_bf16_bwd(const vcg_conv_desc* d, const void* u, const void* wfrag, const void* bias, const void* m, const void* dy,
                                 const void* dres, void* dm, void* da, hipStream_t stream) {
    return gate_bwd(d, true, u, wfrag, bias, m, dy, dres, dm, da, stream);
}

int vcg_conv9x9_from3_bf16_fwd(const vcg_conv_desc* d, const void* x, const void* wfrag, const void* bias, const void* prelu_alpha,
                               void* y, hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(x);
    VCG_CHECK_PTR(wfrag);
    VCG_CHECK_PTR(y);
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->oh != d->h || d->ow != d->w) return VCG_E_SHAPE;
    if (d->cin != 3 || d->kh != 9 || d->kw != 9 || d->stride != 1 || d->pad_top != 4 || d->pad_left != 4) return VCG_E_UNSUPPORTED;
    return launch_conv9x9_3ch(d, d->cout, x, wfrag, bias, prelu_alpha, nullptr, 0.f, y, nullptr, stream);
}

int vcg_conv9x9_from3_bf16_fwd_train(const vcg_conv_desc* d, const void* x, const void* wfrag, const void* bias, const void* prelu_alpha,
                                     void* y, void* z, hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(x);
    VCG_CHECK_PTR(wfrag);
    VCG_CHECK_PTR(y);
    VCG_CHECK_PTR(z);
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->oh != d->h || d->ow != d->w) return VCG_E_SHAPE;
    if (d->cin != 3 || d->kh != 9 || d->kw != 9 || d->stride != 1 || d->pad_top != 4 || d->pad_left != 4) return VCG_E_UNSUPPORTED;
    return launch_conv9x9_3ch(d, d->cout, x, wfrag, bias, prelu_alpha, nullptr, 0.f, y, nullptr, stream, z);
}

int vcg_conv9x9_to3_bf16_dgrad(const vcg_conv_desc* d, const void* dy, const void* wfrag, const void* y_prev, float lrelu_slope, void* dx,
                               hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(dy);
    VCG_CHECK_PTR(wfrag);
    VCG_CHECK_PTR(dx);
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->oh != d->h || d->ow != d->w) return VCG_E_SHAPE;
    if (d->cout != 3 || d->kh != 9 || d->kw != 9 || d->stride != 1 || d->pad_top != 4 || d->pad_left != 4) return VCG_E_UNSUPPORTED;
    return launch_conv9x9_3ch(d, d->cin, dy, wfrag, nullptr, nullptr, y_prev, lrelu_slope, dx, nullptr, stream);
}

// the same, also leaving per-channel sums of the stored dx as records [vcg_conv9x9_to3_bf16_dgrad_chsum_records(d)][cin] -- the bias gradient of
// the layer that produced the convolution's input (upsampling_block's Conv2DTranspose, model.py:72) without another pass over dx; add the
// records up with vcg_sum_records
int vcg_conv9x9_to3_bf16_dgrad_chsum_records(const vcg_conv_desc* d) {
    if (d == nullptr) return VCG_E_NULL;
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->cin <= 0 || d->cin % 64) return VCG_E_SHAPE;
    return conv9x9_3ch_wgs(d, d->cin) * NCW;
}

int vcg_conv9x9_to3_bf16_dgrad_chsum(const vcg_conv_desc* d, const void* dy, const void* wfrag, const void* y_prev, float lrelu_slope, void* dx,
                                     float* records, hipStream_t stream) {
    VCG_CHECK_PTR(d);
    VCG_CHECK_PTR(dy);
    VCG_CHECK_PTR(wfrag);
    VCG_CHECK_PTR(dx);
    VCG_CHECK_PTR(records);
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->oh != d->h || d->ow != d->w) return VCG_E_SHAPE;
    if (d->cout != 3 || d->kh != 9 || d->kw != 9 || d->stride != 1 || d->pad_top != 4 || d->pad_left != 4) return VCG_E_UNSUPPORTED;
    return launch_conv9x9_3ch(d, d->cin, dy, wfrag, nullptr, nullptr, y_prev, lrelu_slope, dx, records, stream);
}

}  // extern "C"
