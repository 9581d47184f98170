// run_split_kernels.hip -- the splitting of touching glyphs on the device (gfx950): k_run_cuts finds the cut columns and the atoms of
// every glyph run from its column profile, k_split_words chooses the segmentation of every run of a word from the cost rows of its
// pieces.  Integers only and no atomics: the output is the same bytes every time.  The rules are stated for the host in
// run_split_rules.h; the contract is at str_er_run_split in str_er.h.
//
// k_run_cuts: a workgroup a line, a wave a run of it (the runs wave, wave + RS_WAVES, ..), working from the run slots k_foot_words has
// just written: no table of the host's.  A lane takes a column of a block of 64 columns: the row word the block's columns lie in is
// one address for the whole wave (two words merged where the run's first column is not word-aligned), and every lane tests its own bit
// of it, counting and keeping the first and last row.  The profile (counts, tops, bottoms: 16 bits each, a box is at most 16384 rows) of
// up to RS_MAX_W columns lies in the wave's own LDS rows.  The low columns of a block are one ballot; the wave walks the intervals of
// the ballots with scalar bit scans, carrying an interval that runs on into the next block, and takes depth, first and last deepest
// column of a valley as two wave minima over keys (count << 16 | column, count << 16 | 0xFFFF - column).  The three smallest
// (depth << 16 | column) keys are kept sorted in three registers.  The atoms' pixels and row extents are wave reductions of per-lane
// sums selected by constant atom numbers: no array is indexed at run time and nothing spills.
//
// k_split_words: a wave a word, a run of it after the other.  The minimum of a 65-byte row is a wave minimum (lane a the byte a, lane 0
// the last as well); the recurrence over at most 4 atoms is unrolled over constant (i, j), its D and predecessors in registers picked
// by compare chains, and the same values in every lane.  The rows of the chosen parts are copied, a lane a byte.
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "../../include/str_er.h"
#include "run_split_kernels.h"

namespace str_er {

namespace {

static_assert(sizeof(str_er_run_split) == 32 && offsetof(str_er_run_split, n_cuts) == 0 && offsetof(str_er_run_split, first_piece) == 20,
              "str_er_run_split layout (host and device)");
static_assert(sizeof(str_er_run_piece) == 32 && sizeof(str_er_split_part) == 8 && sizeof(str_er_word_split) == 16, "run split records (host and device)");

constexpr int RS_THREADS = 64 * RS_WAVES;
constexpr int RS_ROW = 65;

// what one lane writes another lane of the same wave reads: the wave runs in lockstep and its LDS operations complete in order
__device__ __forceinline__ void rs_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t rs_wave_min(uint32_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off, 64));
    return v;
}
__device__ __forceinline__ uint32_t rs_wave_max(uint32_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off, 64));
    return v;
}
__device__ __forceinline__ uint32_t rs_wave_sum(uint32_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}

constexpr uint32_t RS_NONE = 0xFFFFFFFFu;

__global__ void __launch_bounds__(RS_THREADS) k_run_cuts(const FootLine *__restrict__ lines, int n_lines, const WordsSlot *__restrict__ slots,
                                                         const WordsRec *__restrict__ recs, const WordsRun *__restrict__ runs,
                                                         const uint64_t *__restrict__ feet, int num, int den, RunCutRec *__restrict__ out)
{
    __shared__ uint16_t s_cnt[RS_WAVES][RS_MAX_W], s_top[RS_WAVES][RS_MAX_W], s_bot[RS_WAVES][RS_MAX_W];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    uint16_t *cnt_w = s_cnt[wave], *top_w = s_top[wave], *bot_w = s_bot[wave];
    for (int a = (int)blockIdx.x; a < n_lines; a += (int)gridDim.x) {
        const FootLine  L = lines[a];
        const WordsSlot S = slots[a];
        if (L.w <= 0 || L.h <= 0 || L.w > WORDS_MAX_BOX || L.h > WORDS_MAX_BOX || (uint64_t)L.pitch * 64u < (uint64_t)L.w) continue;
        const uint32_t  n_runs = min(recs[a].n_runs, S.cap);
        const uint32_t  P = L.pitch;
        const uint64_t *box = feet + L.word_off;
        for (uint32_t k = (uint32_t)wave; k < n_runs; k += RS_WAVES) {
            const WordsRun *R = runs + S.first + k;
            RunCutRec      *O = out + S.first + k;
            const int x0 = __builtin_amdgcn_readfirstlane(R->x0), x1 = __builtin_amdgcn_readfirstlane(R->x1);
            const int y0 = __builtin_amdgcn_readfirstlane(R->y0), y1 = __builtin_amdgcn_readfirstlane(R->y1);
            const int W = x1 - x0, H = y1 - y0, c0 = x0 - L.x, r0 = y0 - L.y;
            uint32_t  key0 = RS_NONE, key1 = RS_NONE, key2 = RS_NONE;          // depth << 16 | column of the kept valleys, ascending
            uint32_t  px0 = 0, px1 = 0, px2 = 0, px3 = 0, t0 = 0xFFFFu, t1 = 0xFFFFu, t2 = 0xFFFFu, t3 = 0xFFFFu, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
            // (the run inside its line's box: the rows and columns read below)
            const bool inside = W > 0 && H > 0 && c0 >= 0 && r0 >= 0 && c0 + W <= L.w && r0 + H <= L.h;
            const uint32_t thr = inside ? (uint32_t)((int64_t)H * num / den) : 0u;
            if (inside && W <= RS_MAX_W) {
                const int nb = (W + 63) >> 6;
                for (int b = 0; b < nb; ++b) {
                    const uint32_t fc = (uint32_t)c0 + 64u * (uint32_t)b, j = fc >> 6, sh = fc & 63u;
                    const bool     two = sh != 0u && j + 1u < P;          // (the block's columns straddle two words)
                    uint32_t       n = 0, top = 0xFFFFu, bot = 0;
#pragma unroll 4
                    for (int r = 0; r < H; ++r) {
                        const uint64_t *rw = box + (uint64_t)(r0 + r) * P + j;
                        uint64_t v = rw[0] >> sh;
                        if (two) v |= rw[1] << (64u - sh);
                        if ((v >> lane) & 1ull) { ++n; top = min(top, (uint32_t)r); bot = (uint32_t)r + 1u; }
                    }
                    const int c = 64 * b + lane;
                    if (c < W) { cnt_w[c] = (uint16_t)n; top_w[c] = (uint16_t)top; bot_w[c] = (uint16_t)bot; }
                }
                rs_wave_sync();
                // the valleys: the intervals of low columns that touch neither end
                int open = -1;
                for (int b = 0; b < nb; ++b) {
                    const int      c = 64 * b + lane;
                    const uint64_t m = __ballot(c < W && (uint32_t)cnt_w[c] <= thr);
                    for (int pos = 0; pos < 64;) {
                        if (open < 0) {
                            const uint64_t t = m >> pos;
                            if (!t) break;
                            pos += __builtin_ctzll(t);
                            open = 64 * b + pos;
                        }
                        const uint64_t z = ~m >> pos;          // (the bits shifted in are 0: an interval up to the block's end goes on)
                        if (!z) break;
                        pos += __builtin_ctzll(z);
                        const int va = open, vb = 64 * b + pos;
                        open = -1;
                        if (va == 0 || vb >= W) continue;
                        uint32_t kf = RS_NONE, kl = RS_NONE;
                        for (int q = va + lane; q < vb; q += 64) {
                            const uint32_t nq = cnt_w[q];
                            kf = min(kf, nq << 16 | (uint32_t)q);
                            kl = min(kl, nq << 16 | (0xFFFFu - (uint32_t)q));
                        }
                        kf = rs_wave_min(kf); kl = rs_wave_min(kl);
                        const uint32_t cf = kf & 0xFFFFu, cl = 0xFFFFu - (kl & 0xFFFFu);
                        const uint32_t key = (kf & 0xFFFF0000u) | ((cf + cl) >> 1);
                        if (key < key0) { key2 = key1; key1 = key0; key0 = key; }
                        else if (key < key1) { key2 = key1; key1 = key; }
                        else if (key < key2) key2 = key;
                    }
                }
                // the kept cuts by column, the unused ones behind every column
                uint32_t p0 = key0 == RS_NONE ? 0x7FFFFFFFu : key0 & 0xFFFFu, p1 = key1 == RS_NONE ? 0x7FFFFFFFu : key1 & 0xFFFFu;
                uint32_t p2 = key2 == RS_NONE ? 0x7FFFFFFFu : key2 & 0xFFFFu;
                { const uint32_t lo = min(p0, p1), hi = max(p0, p1); p0 = lo; p1 = hi; }
                { const uint32_t lo = min(p1, p2), hi = max(p1, p2); p1 = lo; p2 = hi; }
                { const uint32_t lo = min(p0, p1), hi = max(p0, p1); p0 = lo; p1 = hi; }
                key0 = p0; key1 = p1; key2 = p2;
                for (int c = lane; c < W; c += 64) {
                    const uint32_t at = (uint32_t)((uint32_t)c >= p0) + (uint32_t)((uint32_t)c >= p1) + (uint32_t)((uint32_t)c >= p2);
                    const uint32_t nq = cnt_w[c], tq = top_w[c], bq = bot_w[c];
                    if (at == 0u) { px0 += nq; t0 = min(t0, tq); b0 = max(b0, bq); }
                    else if (at == 1u) { px1 += nq; t1 = min(t1, tq); b1 = max(b1, bq); }
                    else if (at == 2u) { px2 += nq; t2 = min(t2, tq); b2 = max(b2, bq); }
                    else { px3 += nq; t3 = min(t3, tq); b3 = max(b3, bq); }
                }
                px0 = rs_wave_sum(px0); px1 = rs_wave_sum(px1); px2 = rs_wave_sum(px2); px3 = rs_wave_sum(px3);
                t0 = rs_wave_min(t0); t1 = rs_wave_min(t1); t2 = rs_wave_min(t2); t3 = rs_wave_min(t3);
                b0 = rs_wave_max(b0); b1 = rs_wave_max(b1); b2 = rs_wave_max(b2); b3 = rs_wave_max(b3);
                rs_wave_sync();          // (the wave's reads of its LDS rows before its next run writes them)
            } else {          // not split: the run is its one atom
                key0 = key1 = key2 = 0x7FFFFFFFu;
                px0 = R->pixels; t0 = 0; b0 = (uint32_t)max(H, 0);
            }
            if (lane == 0) {
                const int n_cuts = (int)(key0 != 0x7FFFFFFFu) + (int)(key1 != 0x7FFFFFFFu) + (int)(key2 != 0x7FFFFFFFu);
                O->n_cuts = n_cuts;
                O->cut[0] = n_cuts > 0 ? x0 + (int)key0 : -1; O->cut[1] = n_cuts > 1 ? x0 + (int)key1 : -1; O->cut[2] = n_cuts > 2 ? x0 + (int)key2 : -1;
                O->thr = thr;
                O->px[0] = px0; O->y0[0] = y0 + (int)t0; O->y1[0] = y0 + (int)b0;
                O->px[1] = n_cuts > 0 ? px1 : 0u; O->y0[1] = n_cuts > 0 ? y0 + (int)t1 : 0; O->y1[1] = n_cuts > 0 ? y0 + (int)b1 : 0;
                O->px[2] = n_cuts > 1 ? px2 : 0u; O->y0[2] = n_cuts > 1 ? y0 + (int)t2 : 0; O->y1[2] = n_cuts > 1 ? y0 + (int)b2 : 0;
                O->px[3] = n_cuts > 2 ? px3 : 0u; O->y0[3] = n_cuts > 2 ? y0 + (int)t3 : 0; O->y1[3] = n_cuts > 2 ? y0 + (int)b3 : 0;
                O->pad = 0;
            }
        }
    }
}

// the minimum of a cost row: lane a the byte a, lane 0 the last one as well
__device__ __forceinline__ int32_t rs_row_min(const uint8_t *row, int lane)
{
    uint32_t v = row[lane];
    if (lane == 0) v = min(v, (uint32_t)row[64]);
    return (int32_t)rs_wave_min(v);
}

// the piece (i, j) of a run of A atoms in the order by (i, j) without (0, A); -1: the run itself
__device__ __forceinline__ int rs_piece_index(int A, int i, int j)
{
    if (i == 0) return j == A ? -1 : j - 1;
    return (A - 1) + (i - 1) * A - (i - 1) * i / 2 + (j - i - 1);
}

__global__ void __launch_bounds__(RS_THREADS) k_split_words(const str_er_run_split *__restrict__ splits, const uint8_t *__restrict__ run_costs,
                                                            const uint8_t *__restrict__ piece_costs, const int32_t *__restrict__ first_run,
                                                            const int32_t *__restrict__ n_of, const int32_t *__restrict__ slot, int n_words, int split,
                                                            int32_t *__restrict__ word_out, int32_t *__restrict__ parts, uint8_t *__restrict__ part_costs,
                                                            int32_t *__restrict__ n_parts_out)
{
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int w = (int)blockIdx.x * RS_WAVES + wave;
    if (w >= n_words) return;
    const int first = __builtin_amdgcn_readfirstlane(first_run[w]), m = max(0, __builtin_amdgcn_readfirstlane(n_of[w]));
    const size_t base = (size_t)__builtin_amdgcn_readfirstlane(slot[w]);
    int     n_parts = 0;
    int32_t cost = 0, read_cost = 0;
    for (int r = first; r < first + m; ++r) {
        const int      A = min(max(__builtin_amdgcn_readfirstlane(splits[r].n_cuts), 0), 3) + 1;
        const int      fp = __builtin_amdgcn_readfirstlane(splits[r].first_piece);
        const uint8_t *rrow = run_costs + (size_t)r * RS_ROW;
        int32_t D[5];
        int     P[5];
        int32_t own = 0;
        D[0] = 0; P[0] = 0;
#pragma unroll
        for (int j = 1; j <= 4; ++j) {
            int32_t best = 0x7FFFFFFF;
            int     pred = 0;
            if (j <= A) {
#pragma unroll
                for (int i = 0; i < j; ++i) {
                    const int      k = rs_piece_index(A, i, j);
                    const int32_t  mn = rs_row_min(k < 0 ? rrow : piece_costs + ((size_t)fp + (size_t)k) * RS_ROW, lane);
                    const int32_t  v = D[i] + mn + (i > 0 ? split : 0);
                    if (k < 0) own = mn;
                    if (v < best) { best = v; pred = i; }
                }
            }
            D[j] = best; P[j] = pred;
        }
        // the backtrack from A: the parts from the last to the first
        int F[4], T[4];
        int j = A, np = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            F[s] = 0; T[s] = 0;
            if (j > 0) {
                const int i = j == 1 ? P[1] : j == 2 ? P[2] : j == 3 ? P[3] : P[4];
                F[s] = i; T[s] = j;
                j = i; ++np;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (s < np) {
                const int      k = rs_piece_index(A, F[s], T[s]);
                const size_t   at = base + (size_t)(n_parts + np - 1 - s);
                const uint8_t *row = k < 0 ? rrow : piece_costs + ((size_t)fp + (size_t)k) * RS_ROW;
                part_costs[at * RS_ROW + lane] = row[lane];
                if (lane == 0) {
                    part_costs[at * RS_ROW + 64] = row[64];
                    parts[2 * at] = r; parts[2 * at + 1] = k < 0 ? -1 : fp + k;
                }
            }
        n_parts += np;
        cost += A == 1 ? D[1] : A == 2 ? D[2] : A == 3 ? D[3] : D[4];
        read_cost += own;
    }
    if (lane == 0) {
        word_out[4 * (size_t)w] = n_parts; word_out[4 * (size_t)w + 1] = cost; word_out[4 * (size_t)w + 2] = read_cost; word_out[4 * (size_t)w + 3] = 0;
        if (n_parts_out) n_parts_out[w] = n_parts;          // (the run count of the word's window for the matcher and the decoder)
    }
}

} // namespace

void launch_run_cuts(hipStream_t s, const FootLine *lines, int n_lines, const WordsSlot *slots, const WordsRec *recs, const WordsRun *runs,
                     const uint64_t *feet, int num, int den, RunCutRec *out)
{
    if (n_lines <= 0) return;
    hipLaunchKernelGGL(k_run_cuts, dim3((unsigned)(n_lines < (1 << 16) ? n_lines : 1 << 16)), dim3(RS_THREADS), 0, s, lines, n_lines, slots, recs, runs, feet,
                       num, den, out);
}

void launch_split_words(hipStream_t s, const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of,
                        const int32_t *slot, int n_words, int split, int32_t *word_out, int32_t *parts, uint8_t *part_costs, int32_t *n_parts_out)
{
    if (n_words <= 0) return;
    hipLaunchKernelGGL(k_split_words, dim3((unsigned)((n_words + RS_WAVES - 1) / RS_WAVES)), dim3(RS_THREADS), 0, s, splits,
                       run_costs, piece_costs, first_run, n_of, slot, n_words, split, word_out, parts, part_costs, n_parts_out);
}

} // namespace str_er
