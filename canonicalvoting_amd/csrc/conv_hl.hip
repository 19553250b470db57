// conv_hl: the fp16-pair sparse convolution on hl-format activations (the eval network's kernel below conv_hd's row
// threshold, and on every coarse level), with its launcher.  When it runs is decided in sparse_conv.hip.
#include "cv_common.h"

#include <algorithm>

#include "sparse_conv_common.h"

using namespace cvsc;

namespace {

// ------------------------------------------------------------------ fp16-pair convolution on hl-format activations
// conv_rows_wp's tiling (128 rows x NB*32 columns, a wave owns 32 rows, weight tile shared through LDS, one workgroup
// barrier per (offset, 32-channel) unit) with the gathered operand taken straight from global memory: in the hl format
// a lane's MFMA A fragments of a unit are four contiguous 16-byte pieces of its row's 128-byte chunk, so the gather IS
// the fragment load - no fp16 split (it was 2/3 of the VALU work of conv_rows_wp: 17.8 VALU instructions per MFMA,
// profiles/r1/conv_pmc_wp.txt), no LDS staging of A, no in_max scan.  That frees the registers for a deeper software
// pipeline: two units' fragments are in flight (conv_rows_wp: one, and the wave-time ablations of round 2,
// profiles/r2/hl_ablate_trace.txt, put most of the small layers' 20 us in that dependent chain of load round trips).
// Same units, same MFMA sequence per accumulator as conv_rows_wp on the same h / l
// pieces: bit-identical accumulators.
// Two unit slots (registers for the A fragments and this thread's share of the weight tile, one LDS weight tile each):
// the loads of unit u + 2 are requested once unit u has multiplied.  Workgroups of the split coarse levels have no more
// than two units: all their loads are in flight after the prologue (two dependent round trips - map entries, fragments -
// instead of one per unit).  Four waves = 128 rows per workgroup.
// (Measured and removed, git fdb3db3 holds the code: one and three unit slots, 8-wave workgroups - profiles/r2/hl_slots.txt,
// hl_nw8.txt, LABNOTES "Round 3" - and the line-coalesced gather through a wave-private LDS tile: bit-identical, net
// 2.445 -> 2.54 ms, 506 -> 475 scenes/s six in flight, profiles/r3/hl_coal_ab.txt - the LDS round trip on every unit's
// critical path costs more than the faster gather returns.)
// The unit walk is resolved once, before the loop: wave 0 compacts the workgroup's live (offset, chunk) units into a
// list in LDS, the loop is a counted loop over that list with per-thread invariants (weight-tile source / LDS offsets,
// 32-bit row offsets) hoisted - the first version spent ~150 vector and ~250 scalar instructions per unit on the walk
// (advance / skip_dead, 64-bit address arithmetic, spilled scalars) around 18 MFMAs.
// workgroups per CU the register allocation aims at (the second __launch_bounds__ argument; the waves-per-SIMD attribute
// restates it, because an explicit amdgpu_waves_per_eu replaces the bound __launch_bounds__ implies - a (1, 8) range
// silently cost the 96-column kernel a workgroup per CU for most of round 3)
constexpr int hl_blocks(int NB) { return NB <= 3 ? 4 : 2; }
// MA: empty - the kernel as it always was - or one ModelArgs (the model axis of cv_net_run_models_f32, a separate
// instantiation): blockIdx.y = model * ma.ncb + column block, and model_enter swaps the model's operands into `a` at entry.
template <int NB, class... MA>
__global__ __attribute__((amdgpu_waves_per_eu(hl_blocks(NB), 8)))
__launch_bounds__(THREADS, hl_blocks(NB)) void conv_hl(ConvArgs a, MA... ma) {
    const unsigned by = model_enter(a, blockIdx.y, ma...);                  // column block
    constexpr int NS = 2, NW = THREADS / 64;                                // unit slots, waves
    constexpr int B_BYTES = 2 * NB * 32 * 64, EP_BYTES = NW * 32 * EP_LD * 4;
    constexpr int SM_BYTES = NS * B_BYTES > EP_BYTES ? NS * B_BYTES : EP_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char sm[SM_BYTES];     // NS x weight tile [plane][col][64 B]; then the epilogue tile
    __shared__ int rows_s[TM];
    __shared__ int nbr_all[WP_NPRE + 1][TM];
    __shared__ unsigned wave_mask[NW];
    __shared__ unsigned short units_s[HL_MAX_UNITS + 4];      // (jj << 8) | chunk of every live unit, in processing order; [HL_MAX_UNITS] = count
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = by * (NB * 32);
    const long long tile_id = tile_of(a);
    const int half = lane >> 5, l31 = lane & 31;
    const int nj = a.j_end - a.j_begin;
    const int nch = a.cin / KC;
    int u_lo, u_hi;
    if (a.perm_per_split) {
        u_lo = (int)((long long)nj * blockIdx.z / a.splits) * nch;
        u_hi = (int)((long long)nj * (blockIdx.z + 1) / a.splits) * nch;
    } else {
        u_lo = (int)((long long)nj * nch * blockIdx.z / a.splits);
        u_hi = (int)((long long)nj * nch * (blockIdx.z + 1) / a.splits);
    }
    const int j_first = a.j_begin + u_lo / nch, j_last = a.j_begin + (u_hi - 1) / nch;
    const int njl = u_hi > u_lo ? j_last - j_first + 1 : 0;       // <= WP_NPRE (host)
    const int nch2 = a.in2 ? a.cin2 / KC : 0;

    // order and map entries in one phase (independent unless a single order comes without its map rows), one barrier
    const int* perm = a.row_perm ? a.row_perm + (a.perm_per_split ? (long long)blockIdx.z * a.n_out : 0) : nullptr;
    if (tid < TM) {
        const long long t = tile_id * TM + tid;
        const int row = t < a.n_out ? (perm ? perm[t] : (int)t) : -1;
        rows_s[tid] = row;
        if (a.in2) nbr_all[njl][tid] = row;
    }
    {
        unsigned m = 0u;
        const int jg0 = a.j_begin + (int)((long long)nj * blockIdx.z / a.splits);      // first offset of this mask group
        for (int e = tid; e < njl * TM; e += THREADS) {
            const int jj = e / TM, t = e - jj * TM;
            const long long pos = tile_id * TM + t;
            int v = -1;
            if (pos < a.n_out) {
                if (a.nbr_perm) {
                    v = a.nbr_perm[((long long)blockIdx.z * a.n_out + pos) * a.nbr_perm_w + (j_first + jj - jg0)];
                } else {
                    const int row = perm ? perm[pos] : (int)pos;
                    v = a.nbr ? a.nbr[(long long)row * a.K + j_first + jj] : row;
                }
            }
            nbr_all[jj][t] = v;
            if (v >= 0) m |= 1u << jj;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m |= __shfl_xor(m, off);
        if (lane == 0) wave_mask[wave] = m;
    }
    __syncthreads();
    unsigned lm = 0u;
#pragma unroll
    for (int w = 0; w < NW; ++w) lm |= wave_mask[w];
    if (wave == 0) {
        // live units of the map in order, then the chunks of the second source dealt to this split
        const int n_first = u_hi - u_lo, n_second = nch2 > (int)blockIdx.z ? (nch2 - (int)blockIdx.z + a.splits - 1) / a.splits : 0;
        int cnt = 0;
        for (int base = 0; base < n_first + n_second; base += 64) {
            const int e = base + lane;
            int code = -1;
            if (e < n_first) {
                const int u = u_lo + e, q = u / nch;
                const int jj = a.j_begin + q - j_first;
                if ((lm >> jj) & 1u) code = (jj << 8) | (u - q * nch);
            } else if (e < n_first + n_second) {
                code = (njl << 8) | ((int)blockIdx.z + (e - n_first) * a.splits);
            }
            const unsigned long long bal = __ballot(code >= 0);
            if (code >= 0) units_s[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)code;
            cnt += __popcll(bal);
        }
        if (lane == 0) units_s[HL_MAX_UNITS] = (unsigned short)cnt;
    }
    __syncthreads();
    const int n_units = __builtin_amdgcn_readfirstlane((int)units_s[HL_MAX_UNITS]);
    if (n_units == 0 && a.gvalid) return;            // no row of the tile has a neighbour in this group: nothing to write (zskip)

    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;

    // per-thread invariants of the weight tile: this thread's 16-byte pieces (source offset inside a unit's slab in 16-bit
    // words, or -1 beyond Cout; LDS offset with the XOR swizzle)
    constexpr int B_U4 = 2 * NB * 32 * 4;
    constexpr int B_PER = (B_U4 + THREADS - 1) / THREADS;
    int b_src[B_PER], b_dst[B_PER];
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
        const int f = tid + i * THREADS;
        const int p = f / (NB * 32 * 4), rem = f - p * (NB * 32 * 4);
        const int col = rem >> 2, ch = rem & 3;
        b_src[i] = (f < B_U4 && n0 + col < a.cout) ? (p * a.cout + n0 + col) * 32 + ch * 8 : -1;
        b_dst[i] = f < B_U4 ? (p * NB * 32 + col) * 64 + ((ch ^ ((col >> 2) & 3)) << 4) : -1;
    }
    const unsigned slab_words = 2u * (unsigned)a.cout * 32u;       // one unit's slab: [plane][cout][32] 16-bit words
    const int my_row = wave * 32 + l31;
    const unsigned in_row_bytes = (unsigned)a.in_ld * 4u, in2_row_bytes = (unsigned)a.in2_ld * 4u;
    const unsigned char* const in_b = reinterpret_cast<const unsigned char*>(a.in);
    const unsigned char* const in2_b = reinterpret_cast<const unsigned char*>(a.in2);

    uint4 ra[NS][4], rb[NS][B_PER];
    bool live[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) live[q] = false;
    auto load = [&](auto S, int k) {                  // unit k of the list -> slot S
        constexpr int sl = decltype(S)::value;
        const int code = __builtin_amdgcn_readfirstlane((int)units_s[k]);
        const int jj = code >> 8, c = code & 255;
        const bool second = jj == njl;
        const int src = nbr_all[jj][my_row];
        live[sl] = __any(src >= 0);
        if (src >= 0) {
            const unsigned off = (unsigned)src * (second ? in2_row_bytes : in_row_bytes) + (unsigned)(c * 128 + half * 16);
            const unsigned char* p = (second ? in2_b : in_b) + off;
            ra[sl][0] = *reinterpret_cast<const uint4*>(p);
            ra[sl][1] = *reinterpret_cast<const uint4*>(p + 32);
            ra[sl][2] = *reinterpret_cast<const uint4*>(p + 64);
            ra[sl][3] = *reinterpret_cast<const uint4*>(p + 96);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) ra[sl][q] = make_uint4(0u, 0u, 0u, 0u);
        }
        const unsigned short* slab = second ? a.wp6_2 + (size_t)c * slab_words
                                            : a.wp6 + (size_t)((j_first + jj) * nch + c) * slab_words;
#pragma unroll
        for (int i = 0; i < B_PER; ++i)
            rb[sl][i] = b_src[i] >= 0 ? *reinterpret_cast<const uint4*>(slab + b_src[i]) : make_uint4(0u, 0u, 0u, 0u);
    };
    auto stage_b = [&](auto S, int toff) {            // toff: byte offset of the LDS weight tile (slot * B_BYTES)
        constexpr int sl = decltype(S)::value;
#pragma unroll
        for (int i = 0; i < B_PER; ++i)
            if (b_dst[i] >= 0) *reinterpret_cast<uint4*>(sm + toff + b_dst[i]) = rb[sl][i];
    };
    const int b_rd = l31 * 64;
    const int bswz = (l31 >> 2) & 3;
    auto compute = [&](auto S, int toff) {
        constexpr int sl = decltype(S)::value;
        const unsigned char* Bb = sm + toff + b_rd;
        uint4 (&fa)[4] = ra[sl];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int piece = ((2 * ks + half) ^ bswz) << 4;
            const f16x8 a0 = __builtin_bit_cast(f16x8, fa[ks]), a1 = __builtin_bit_cast(f16x8, fa[2 + ks]);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const f16x8 b0 = *reinterpret_cast<const f16x8*>(Bb + nb * 32 * 64 + piece);
                const f16x8 b1 = *reinterpret_cast<const f16x8*>(Bb + (NB * 32 + nb * 32) * 64 + piece);
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[nb], 0, 0, 0);
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[nb], 0, 0, 0);
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[nb], 0, 0, 0);
                if constexpr (NB >= 3) asm volatile("" ::: "memory");   // keep the next fragments' reads behind these MFMAs (registers)
            }
        }
    };
    typedef std::integral_constant<int, 0> S0;
    typedef std::integral_constant<int, 1> S1;
    if (n_units > 0) load(S0{}, 0);
    if (n_units > 1) load(S1{}, 1);
    if (n_units > 0) stage_b(S0{}, 0);
    // step: unit k in slot s.  barrier: tile k visible, tile k - 1 consumed by everyone; the tile of unit k + 1 goes to LDS;
    // MFMAs of unit k; the registers of unit k take the loads of unit k + 2 once its MFMAs are issued (85 / 113 / 128 VGPRs for
    // 32 / 64 / 96 columns: four workgroups per CU; net 2.53 -> 2.48 ms against three slots for the first two, 2.52 -> 2.48 ms for
    // the third once a compiler barrier keeps its fragment reads from being hoisted - its remaining spills are outside the
    // unit loop)
    auto step = [&](auto S, auto SN, int k) {
        constexpr int sl = decltype(S)::value;
        __syncthreads();
        if (k + 1 < n_units) stage_b(SN, decltype(SN)::value * B_BYTES);
        if (live[sl]) compute(S, sl * B_BYTES);
        if (k + 2 < n_units) load(S, k + 2);
    };
#pragma unroll 1
    for (int k = 0; k < n_units; k += 2) {
        step(S0{}, S1{}, k);
        if (k + 1 >= n_units) break;
        step(S1{}, S0{}, k + 1);
    }
    __syncthreads();                                 // weight tiles are dead: the epilogue tile reuses their LDS
    model_epilogue(a, blockIdx.y, ma...);
    {
        const float sc = a.acc_scale_dev ? a.acc_scale * *a.acc_scale_dev : a.acc_scale;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nb][r] *= sc;
    }
    float (*ep)[EP_LD] = reinterpret_cast<float (*)[EP_LD]>(sm + wave * 32 * EP_LD * 4);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) epilogue_store_wide(a, acc[nb], rows_s + wave * 32, n0 + nb * 32, lane, ep);
    if (a.splits > 1 && a.tickets) {
        // split-K without a second launch: every workgroup of an output tile publishes its partial tile, the LAST one to
        // arrive sums the partial tiles in split order and runs the epilogue.  Publish = write-through (sc1) stores in the
        // epilogue above -> per-wave vmcnt(0) -> barrier -> one relaxed agent-scope ticket; the last arriver's agent acquire
        // (an L1 invalidate) -> plain loads.  No release fence: the stores are already past the L2 (round 2 published with
        // plain stores + an agent release per workgroup and ran 50 % slower, profiles/r2/fused_finish.txt).
        // Summation order = conv_finish's (four running sums over the splits k % 4, then ((s0 + s1) + s2) + s3):
        // bit-identical to the two-launch path.  The last arriver leaves the counter at zero for the next launch.
        __shared__ int last_flag;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int* ticket = a.tickets + tile_id * gridDim.y + by;
        if (tid == 0) {
            const int old = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last_flag = old == a.splits - 1;
            if (last_flag) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        __syncthreads();
        if (!last_flag) return;
        if (tid == 0) *ticket = 0;
        const long long plane = a.n_out * (long long)a.cout;       // one split's partial tile set
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int col = n0 + nb * 32 + (lane & 7) * 4;
            if (col >= a.cout) continue;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int row = rows_s[wave * 32 + (lane >> 3) + 8 * it];
                if (row < 0) continue;
                const float* p = a.partial + (long long)row * a.cout + col;
                float4 sq[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) sq[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int k0 = 0; k0 < a.splits; k0 += 4) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (k0 + q < a.splits) {
                            const float4 v = *reinterpret_cast<const float4*>(p + (long long)(k0 + q) * plane);
                            sq[q].x += v.x; sq[q].y += v.y; sq[q].z += v.z; sq[q].w += v.w;
                        }
                }
                const float4 x = make_float4(sq[0].x + sq[1].x + sq[2].x + sq[3].x, sq[0].y + sq[1].y + sq[2].y + sq[3].y,
                                             sq[0].z + sq[1].z + sq[2].z + sq[3].z, sq[0].w + sq[1].w + sq[2].w + sq[3].w);
                epilogue_apply4(a, row, col, x);
            }
        }
    }
}

}  // namespace

void cvsc::launch_conv_hl(const ConvArgs& a, int nb, const ModelArgs* ma, dim3 grid, hipStream_t st) {
    with_nb<4>(nb, [&](auto nbc) {
        constexpr int NB = decltype(nbc)::value;
        with_models(ma, [&](auto... m) { conv_hl<NB, decltype(m)...><<<grid, THREADS, 0, st>>>(a, m...); });
    });
}
