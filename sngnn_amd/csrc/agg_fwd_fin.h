// The five forms of the split rows' finalize: inside the main launch (fin_group_batch, fin_stream_row,
// fin_block_pair: called by k_agg_fwd, agg_fwd_roles.h), from scores in HBM scratch (k_agg_fin), the candidate
// tournament (k_agg_fin_cand), one wave per row (k_agg_fin_wave) and the two together with the head role
// (k_agg_fin_mixed).  The pieces they share come first.  Needs agg_fwd_args.h, agg_fwd_head.h, agg_fwd_select.h and
// fwd_plan.h (FINC_WAVES_MAX; which form a call takes is decided there).
#pragma once
#include "agg_fwd_args.h"
#include "agg_fwd_head.h"
#include "agg_fwd_select.h"
#include "fwd_plan.h"

namespace sngnn {

constexpr int FIN_SPIN_MAX = 1 << 19;       // polls of a row's done words before the row is given up (the in-launch forms' comment)
constexpr int FIN_GROUP_WORDS = 3 * CAND_MAX_K;      // LDS words of one row's winners: 32 keys (64 words) | 32 source ids

// candidate q of a row whose first task is t0 (task t0 + q / k, entry q % k of its CAND_MAX_K-slot record) without
// the twenty-instruction division per candidate (eight per lane in flight: their temporaries were the role's spills)
__device__ __forceinline__ unsigned fin_slot(const FwdArgs &a, int t0, int q)
{
    const int t = a.k == 1 ? q : (int)__umulhi((unsigned)q, a.k_magic);
    return (unsigned)(t0 + t) * CAND_MAX_K + (unsigned)(q - t * a.k);       // (n_tasks * 32 < 2^31: int32 edge ids, CHUNK = 128)
}

// static LDS of k_agg_fin, and its workgroup-wide count
struct __align__(16) FinShared {
    int red[2][FIN_BLOCK / 64];
    int wave_off[FIN_BLOCK / 64];
    int nsel;
    int pad[3];
};
static_assert(sizeof(FinShared) % 16 == 0, "keep the dynamic LDS base 16-byte aligned");

__device__ __forceinline__ int block_count(int c, FinShared &sh, int &parity)
{
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    c = wave_sum_i(c);
    if (lane == 0) sh.red[parity][wave] = c;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int w = 0; w < FIN_BLOCK / 64; ++w) tot += sh.red[parity][w];
    parity ^= 1;
    return tot;
}

// a split row's head (FwdArgs::head_sel): the finished mean row sits in LDS (s_row[0, C)); the first lane
// group of wave 0 takes it through head_store_row and the row's entry of head_part is written.
// Called by the whole workgroup, behind the barrier that made s_row complete.
template <int VEC, int G, int R>
__device__ __forceinline__ void fin_row_head(const FwdArgs &a, int i, int p, const float *s_row)
{
    if constexpr (VEC == 4 && R == 1 && (G == 8 || G == 16)) {
        if (threadIdx.x >= 64) return;                         // (wave-uniform)
        const int lane = lane_id();
        const int gid = lane / G, lg = lane % G;
        HeadAcc ha;
        if (gid == 0) {
            Row<VEC, G, R> row;
            const float4 t = *reinterpret_cast<const float4 *>(s_row + (4 * lg < a.C ? 4 * lg : 0));
            row.x[0][0] = t.x; row.x[0][1] = t.y; row.x[0][2] = t.z; row.x[0][3] = t.w;
            head_store_row<VEC, G, R>(a, row, i, lg, (int)a.head_y[i], a.head_sel[i], ha);
        }
        head_write_entry(a, a.head_nmain + p, ha);
    }
}

// The winners of a split row (s_key_w / s_src_w [0, nsel): keys and source ids, in the selection's own order) ->
// the row's weighted sum, its mean and stores, the bookkeeping of the kept edges.  One wave.
// LEAN: the call wants `out` only (k_agg_fwd's note) - no wsel, kept bits or selection lists.
template <int VEC, int G, int R, bool HEAD, typename S = float, bool LEAN = false>
__device__ __forceinline__ void fin_winners_row(const FwdArgs &a, int p, int i, int rs, int deg, int t0, int nsel,
                                                const unsigned long long *s_key_w, const int *s_src_w, int head_yy,
                                                unsigned head_sv)
{
    static_assert(std::is_same<S, float>::value || !HEAD, "the head reads fp32 rows");
    using RowT = Row<VEC, G, R>;
    constexpr int NG = 64 / G;
    const int lane = lane_id();
    const int gid = lane / G, lg = lane % G;
    const bool emit = !LEAN && a.sel_src != nullptr;
    RowT acc;
    acc.zero();
    constexpr int GU = R >= 3 ? 2 : 4;                        // winner rows in flight per lane group
    for (int w0 = 0; w0 < nsel; w0 += GU * NG) {
        RowT x[GU];
        float nj[GU];
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            const int w = min(w0 + u * NG + gid, nsel - 1);
            const int j = s_src_w[w];
            x[u].load(a.rows<S>() + (size_t)j * a.C, a.C, lg);
            nj[u] = a.nrm ? a.nrm[j] : 1.0f;
        }
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            const int w = w0 + u * NG + gid;
            if (w < nsel) acc.axpy(key_score(s_key_w[w]) * nj[u], x[u]);
        }
    }
    if (!LEAN && lane < nsel) {
        const unsigned long long kq = s_key_w[lane];
        const float sq = key_score(kq);
        if (a.wsel) a.wsel[rs + key_index(kq)] = sq;
        if (a.kbits) atomicOr(a.kbits + a.kb_tbase + 4 * t0 + (key_index(kq) >> 5), 1u << (key_index(kq) & 31));
        if (emit) {
            int rk = 0;
            for (int r = 0; r < nsel; ++r) rk += s_key_w[r] > kq;
            a.sel_src[(size_t)i * a.k + rk] = s_src_w[lane];
            a.sel_w[(size_t)i * a.k + rk] = sq;
        }
    }
    acc.reduce_across_groups();
    acc.div((float)deg);
    if constexpr (HEAD) {
        HeadAcc ha;
        if (gid == 0) head_store_row<VEC, G, R>(a, acc, i, lg, head_yy, head_sv, ha);
        head_write_entry(a, a.head_nmain + p, ha);
        return;
    }
    if constexpr (!LEAN) row_epilogue<VEC, G, R>(a, acc, i, lg);
    if (gid == 0) acc.store(a.outs<S>() + (size_t)i * a.C, a.C, lg);
}

// ---------------------------------------------------------------------------
// The split rows' finalize inside the main launch (round 5).  As a launch of its own it was 7.4 us of a 70 us
// step at arxiv size - a dependency chain (candidates -> selection -> 16 rows -> store) of 825 rows on an
// otherwise idle chip, behind a launch boundary - although its inputs exist ~5 us into the main kernel: the tasks
// are every wave's FIRST work item.  So the LAST workgroups of the launch (FwdArgs::main_blocks ..) take no work
// items: they finalize the split rows, each as soon as the row's tasks have published their candidates, while the
// other workgroups stream the wave rows and small rows.  What bounds the role is round trips, not work (an
// agent-scope load comes from memory: 2-3 us under the main roles' traffic), so both forms below keep as many
// rows' loads in flight as the registers hold:
//   * rows of more than 128 candidates (arxiv size: 94, up to 1 584 candidates): two WAVES per row, two rows per
//     workgroup - a wave selects among half of the candidates (512 keys per round, eight per lane, all loads of a
//     round in flight together), the even wave among the pair's winners.  (One wave per row, 96 new candidates per
//     round: 17 dependent round trips for the biggest row - the launch's critical path, 66 us against 48.)
//   * the others: one lane GROUP per row, 64 / G rows per wave at once (fin_group_batch) - the accumulation runs in
//     the order of the one-wave-per-row finalize launch (fin_wave_row), so the rows' bits are the same in both.
//   Progress: a task never waits, and workgroups are dispatched in index order, so whenever a finalize workgroup is
// resident every task's workgroup has been dispatched.  Should that ever not hold the wait is BOUNDED: a row whose
// tasks have not shown up after FIN_SPIN_MAX polls (~1 s) is written as NaN and its waves stop waiting for the
// rows behind it - a loud wrong answer, never a hung GPU.
//   Visibility: tasks store what this role reads (candidate keys / sources) or overwrites (unselected marks, zeroed
// kept-bit words) at agent scope and drain them before the done word; this role loads them at agent scope.
// ---------------------------------------------------------------------------

// Rows [pb, pb + 64 / G) of at most 128 candidates each, one per lane group.  seen (per group): the row's done
// words were all read as done by the batch before (the look-ahead below); on return: whether row pb_next + gid's were.
template <int VEC, int G, int R, typename S = float, bool LEAN = false>
__device__ __forceinline__ void fin_group_batch(const FwdArgs &a, int pb, int pb_next, int *lds_wave, bool &dead,
                                                bool &seen)
{
    using RowT = Row<VEC, G, R>;
    constexpr int NG = 64 / G, NKG = 128 / G;
    constexpr unsigned long long FULL = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
    const int lane = lane_id();
    int gid = lane / G, lg = lane % G;
    // (opaque per call: what depends on the lane only - eight slot offsets, masks, shuffle addresses - was hoisted
    // out of the caller's loop over batches and held in ~50 registers across it: 131 against the kernel's 80)
    asm volatile("" : "+v"(gid), "+v"(lg));
    const int p = pb + gid;
    const bool valid = p < a.n_split;
    const int pc = valid ? p : a.n_split - 1;
    const int4 d = a.rdesc[pc];
    const int i = d.x, rs = d.y, deg = d.z;
    const bool act = valid && (LEAN || !a.skip_row(i));       // (group-uniform; a skipped row's tasks skipped it too)
    const int t0 = a.split_task0[pc], t1 = a.split_task0[pc + 1];
    unsigned long long *s_key = reinterpret_cast<unsigned long long *>(lds_wave + gid * FIN_GROUP_WORDS);
    int *s_src = lds_wave + gid * FIN_GROUP_WORDS + 2 * CAND_MAX_K;
    // wait for the rows' tasks
    bool ready = seen || !act;
    for (int spin = 0; !dead && spin < FIN_SPIN_MAX && !__all(ready); ++spin) {
        bool mine = true;
        for (int t = t0 + lg; t < t1; t += G) mine = mine && ld_agent(a.fin_done + t) == a.fin_nonce;
        ready = ready || fwd_group_bits<G>(__ballot(mine), gid) == FULL;
        if (!__all(ready)) __builtin_amdgcn_s_sleep(16);
    }
    if (!__all(ready)) dead = true;
    const bool run = act && ready;
    if (act && !ready)
        for (int c = lg; c < a.C; c += G) a.out_at<S>((size_t)i * a.C + c) = __uint_as_float(0x7FC00000u);
    if (run)
        for (int t = t0 + lg; t < t1; t += G) st_agent(a.fin_done + t, 0ull);     // consumed (a replayed launch finds zeros)
    // look ahead: the next batch's done words, in flight under this batch's round trips (by now its tasks are
    // long done - one round trip less per batch; a "done" read early stays true: only this wave clears the words)
    bool mine_next = pb_next + gid < a.n_split;
    if (mine_next) {
        const int u0 = a.split_task0[pb_next + gid], u1 = a.split_task0[pb_next + gid + 1];
        for (int t = u0 + lg; t < u1; t += G) mine_next = mine_next && ld_agent(a.fin_done + t) == a.fin_nonce;
    }
    // candidates: slot q = lg + G u of the row
    const int n = (t1 - t0) * a.k;                            // <= 128: the rows behind FwdArgs::n_split_gt_wave
    auto slot = [&](int q) { return fin_slot(a, t0, q); };
    unsigned long long key[NKG];
    int src[NKG];                                             // (with the keys: one round trip, not two)
#pragma unroll
    for (int u = 0; u < NKG; ++u) {
        const int q = lg + G * u;
        const bool in = run && q < n;
        key[u] = in ? ld_agent(a.cand_key + slot(q)) : 0ull;
        src[u] = in ? ld_agent(a.cand_src + slot(q)) : 0;
    }
    bool kp[NKG];
    group_topk_keys_n<G, NKG>(key, a.k, a.lowbits, kp);
    int nsel = 0;                                             // winners in ascending slot order (fin_wave_row's order)
#pragma unroll
    for (int u = 0; u < NKG; ++u) {
        const unsigned long long m = fwd_group_bits<G>(__ballot(kp[u]), gid);
        if (kp[u]) {
            const int o = nsel + __popcll(m & ((1ull << lg) - 1ull));
            s_key[o] = key[u];
            s_src[o] = src[u];
        }
        nsel += __popcll(m);
    }
    wave_lds_sync();
    // the weighted sum, in the order of fin_winners_row: there lane group g adds the winners w = g (mod 64 / G) in
    // ascending order and the groups' sums meet in a butterfly - here ONE group holds those 64 / G partial sums
    RowT part[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) part[g].zero();
    // rows in flight per group: a multiple of 64 / G.  (Eight at R == 1: 84 registers - three spilled, 12-16 bytes of
    // scratch per lane for EVERY wave of the launch - and no faster: 64.6-64.9 against 64.9-65.2 us per forward,
    // while the launch without the role lost 0.4 us to the scratch set-up.)
    constexpr int STEP = R == 1 ? (NG > 4 ? NG : 4) : (R == 2 ? 4 : 2);
    static_assert(STEP % NG == 0, "the partial sum of a winner must be a compile-time index");
    const int nsel_max = wave_max_i(nsel);
    for (int w0 = 0; w0 < nsel_max; w0 += STEP) {
        RowT x[STEP];
        float nj[STEP];
#pragma unroll
        for (int u = 0; u < STEP; ++u) {
            const int j = nsel > 0 ? s_src[min(w0 + u, nsel - 1)] : 0;
            x[u].load(a.rows<S>() + (size_t)j * a.C, a.C, lg);
            nj[u] = a.nrm ? a.nrm[j] : 1.0f;
        }
#pragma unroll
        for (int u = 0; u < STEP; ++u)
            if (w0 + u < nsel) part[u % NG].axpy(key_score(s_key[w0 + u]) * nj[u], x[u]);
    }
    const bool emit = !LEAN && a.sel_src != nullptr;
    for (int w = lg; !LEAN && w < nsel; w += G) {
        const unsigned long long kq = s_key[w];
        const float sq = key_score(kq);
        if (a.wsel) a.wsel[rs + key_index(kq)] = sq;
        if (a.kbits) atomicOr(a.kbits + a.kb_tbase + 4 * t0 + (key_index(kq) >> 5), 1u << (key_index(kq) & 31));
        if (emit) {
            int rk = 0;
            for (int r = 0; r < nsel; ++r) rk += s_key[r] > kq;
            a.sel_src[(size_t)i * a.k + rk] = s_src[w];
            a.sel_w[(size_t)i * a.k + rk] = sq;
        }
    }
#pragma unroll
    for (int m = 1; m < NG; m <<= 1)
#pragma unroll
        for (int g = 0; g < NG; g += 2 * m) part[g].add(part[g + m]);
    part[0].div((float)deg);
    if constexpr (!LEAN) row_epilogue<VEC, G, R>(a, part[0], i, lg);
    if (run) part[0].store(a.outs<S>() + (size_t)i * a.C, a.C, lg);
    seen = fwd_group_bits<G>(__ballot(mine_next), gid) == FULL;
    wave_lds_sync();            // the wave's LDS scratch is reused by its next batch
}

// A split row of a call that selects nothing (top_k < 0: SNConv): the sum of its tasks' partial rows, one wave per
// row, a lane per channel - in the finalize launch's own order (sixteen slices, slice s = tasks s, s + 16, .. added
// in turn, then the slices in order: fin_cand_row / fin_wave_row), sixteen loads in flight.  seen / p_next: the
// look-ahead of fin_group_batch.
template <int VEC, int G, int R, typename S = float>
__device__ __forceinline__ void fin_stream_row(const FwdArgs &a, int p, int p_next, bool &dead, bool &seen)
{
    int lane = lane_id();
    asm volatile("" : "+v"(lane));                          // (opaque per call: fin_group_batch's note)
    const int4 d = a.rdesc[p];
    const int i = d.x, deg = d.z;
    const bool was_seen = seen;
    seen = false;
    if (a.skip_row(i)) return;                              // (wave-uniform; its tasks skipped it too)
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];
    bool ready = was_seen;
    for (int spin = 0; !ready && !dead && spin < FIN_SPIN_MAX; ++spin) {
        bool mine = true;
        for (int t = t0 + lane; t < t1; t += 64) mine = mine && ld_agent(a.fin_done + t) == a.fin_nonce;
        if (__all(mine)) ready = true;
        else __builtin_amdgcn_s_sleep(16);
    }
    if (!ready) {
        dead = true;
        for (int c = lane; c < a.C; c += 64) a.out_at<S>((size_t)i * a.C + c) = __uint_as_float(0x7FC00000u);
        return;
    }
    for (int t = t0 + lane; t < t1; t += 64) st_agent(a.fin_done + t, 0ull);      // consumed (a replayed launch finds zeros)
    bool mine_next = p_next < a.n_split;
    if (mine_next) {
        const int u0 = a.split_task0[p_next], u1 = a.split_task0[p_next + 1];
        for (int t = u0 + lane; t < u1; t += 64) mine_next = mine_next && ld_agent(a.fin_done + t) == a.fin_nonce;
    }
    for (int c0 = 0; c0 < a.C; c0 += 64) {
        const int c = c0 + lane;
        const bool in = c < a.C;
        float sl[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) sl[u] = 0.f;
        for (int tb = t0; tb < t1; tb += 16) {
#pragma unroll
            for (int h = 0; h < 16; h += 8) {                  // (eight loads in flight: sixteen spilled registers)
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    v[u] = (in && tb + h + u < t1) ? ld_agent(a.partial + (size_t)(tb + h + u) * a.C + c) : 0.f;
#pragma unroll
                for (int u = 0; u < 8; ++u) sl[h + u] += v[u];
            }
        }
        float sum = 0.f;
#pragma unroll
        for (int u = 0; u < 16; ++u) sum += sl[u];
        if (in) a.out_at<S>((size_t)i * a.C + c) = a.epilogue(sum / (float)deg, i, c);
    }
    seen = __all(mine_next) != 0;
}

// Two rows of more than 128 candidates each, by the workgroup: waves 0, 1 take the halves of row p0's candidates,
// waves 2, 3 those of row p0 + 1 (none: they only keep the barriers company); the even wave of a pair merges.
// Called by all waves of the workgroup - every wave passes the same three barriers whatever its row's state.
// LDS per wave: its winners' keys [0, 64) words | source ids [64, 96) | count [96] | ready flag [97].
template <int VEC, int G, int R, typename S = float, bool LEAN = false>
__device__ __forceinline__ void fin_block_pair(const FwdArgs &a, int p0, int n_big, int (*lds)[WaveLds<G>::WORDS],
                                               bool &dead)
{
    int lane = lane_id();
    asm volatile("" : "+v"(lane));                          // (opaque per call: fin_group_batch's note)
    const int wave = threadIdx.x >> 6, half = wave & 1;
    int *lw = lds[wave];
    const int p = p0 + (wave >> 1);
    const bool valid = p < n_big;
    const int pc = valid ? p : p0;
    const int4 d = a.rdesc[pc];
    const int i = d.x, rs = d.y, deg = d.z;
    const bool act = valid && (LEAN || !a.skip_row(i));     // (wave-uniform; a skipped row's tasks skipped it too)
    const int t0 = a.split_task0[pc], t1 = a.split_task0[pc + 1];
    unsigned long long *s_key_w = reinterpret_cast<unsigned long long *>(lw);
    int *s_src_w = lw + 2 * CAND_MAX_K;
    // both waves of a pair wait for all of the row's tasks, then they agree
    bool ready = !act;
    for (int spin = 0; !ready && !dead && spin < FIN_SPIN_MAX; ++spin) {
        bool mine = true;
        for (int t = t0 + lane; t < t1; t += 64) mine = mine && ld_agent(a.fin_done + t) == a.fin_nonce;
        if (__all(mine)) ready = true;
        else __builtin_amdgcn_s_sleep(16);
    }
    if (lane == 0) lw[97] = ready ? 1 : 0;
    __syncthreads();
    const bool run = act && ready && lds[wave ^ 1][97] != 0;
    if (act && !run) {
        dead = true;
        if (half == 0)
            for (int c = lane; c < a.C; c += 64) a.out_at<S>((size_t)i * a.C + c) = __uint_as_float(0x7FC00000u);
    }
    if (run && half == 0)
        for (int t = t0 + lane; t < t1; t += 64) st_agent(a.fin_done + t, 0ull);      // consumed (both waves have seen them)
    const int n = (t1 - t0) * a.k;
    auto slot = [&](int q) { return fin_slot(a, t0, q); };
    // this wave's half, in rounds of 512 keys: lanes [0, 32) of the first hold the running winners (k <=
    // CAND_MAX_K = 32), the rest 480 new candidates - all loads of a round in flight together; source ids: the
    // winners' only, behind the selection
    const int per = (n + 1) / 2;
    const int qlo = half * per, qhi = run ? min(n, qlo + per) : qlo;
    constexpr int NK = 8, NEW = 64 * NK - CAND_MAX_K;
    int nsel = 0;
    for (int q0 = qlo; q0 < qhi; q0 += NEW) {
        unsigned long long key[NK];
#pragma unroll
        for (int u = 0; u < NK; ++u) {
            const int q = q0 + u * 64 + lane - CAND_MAX_K;
            const bool in = (u > 0 || lane >= CAND_MAX_K) && q < qhi;
            key[u] = in ? ld_agent(a.cand_key + slot(q)) : 0ull;
        }
        int src_run = 0;
        const bool had = lane < nsel;                      // key[0] is a running winner (its source id is known)
        if (had) { key[0] = s_key_w[lane]; src_run = s_src_w[lane]; }
        wave_lds_sync();                                   // the winners are in registers before their slots are reused
        bool kp[NK];
        wave_topk_keys_n<NK, true>(key, a.k, a.lowbits, kp);
        int off = 0;
#pragma unroll
        for (int u = 0; u < NK; ++u) {
            const unsigned long long m = __ballot(kp[u]);
            if (kp[u]) {
                const int o = off + prefix_popc(m);
                s_key_w[o] = key[u];
                s_src_w[o] = (u == 0 && had) ? src_run : ld_agent(a.cand_src + slot(q0 + u * 64 + lane - CAND_MAX_K));
            }
            off += __popcll(m);
        }
        nsel = off;
        wave_lds_sync();
    }
    if (lane == 0) lw[96] = nsel;
    __syncthreads();
    // the even wave: the pair's winners (<= 32 each) -> one selection
    unsigned long long key0 = 0ull;
    int src0 = 0;
    if (half == 0) {
        const int wa = wave + (lane >> 5), idx = lane & 31;
        if (idx < lds[wa][96]) {
            key0 = reinterpret_cast<const unsigned long long *>(lds[wa])[idx];
            src0 = lds[wa][2 * CAND_MAX_K + idx];
        }
    }
    __syncthreads();                                        // (read before the odd waves reuse their regions)
    if (half != 0 || !run) return;
    bool k0, k1;
    wave_topk_cands(key0, 0ull, a.k, a.lowbits, k0, k1);
    const unsigned long long m0 = __ballot(k0);
    const int nfin = __popcll(m0);
    if (k0) { const int o = prefix_popc(m0); s_key_w[o] = key0; s_src_w[o] = src0; }
    wave_lds_sync();
    fin_winners_row<VEC, G, R, false, S, LEAN>(a, p, i, rs, deg, t0, nfin, s_key_w, s_src_w, 0, 0u);
    wave_lds_sync();
}

// ---------------------------------------------------------------------------
// Finalize of split rows from scores in HBM scratch (top_k > CAND_MAX_K, or a hub whose
// candidates do not fit LDS): one FIN_BLOCK-thread workgroup per row, any degree.
// ---------------------------------------------------------------------------
template <int VEC, int G, int R, typename S = float>
__global__ __launch_bounds__(FIN_BLOCK) void k_agg_fin(const FwdArgs a, int lds_scores)
{
    using RowT = Row<VEC, G, R>;
    constexpr int NG = 64 / G;
    constexpr int NW = FIN_BLOCK / 64;
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ FinShared sh;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const int gid = lane / G, lg = lane % G;
    const int p = blockIdx.x;
    const int i = a.rperm[p];
    if (a.skip_row(i)) return;                              // (workgroup-uniform)
    const int rs = a.rowptr[i];
    const int deg = a.rowptr[i + 1] - rs;
    const bool emit = a.sel_src != nullptr && a.k >= 0;
    const bool rank = a.k >= 0 && deg > a.k;

    // dynamic LDS: [C * NW] partial rows | [k] kept list | [lds_scores] scores
    float *s_part = reinterpret_cast<float *>(dyn);
    int *s_list = reinterpret_cast<int *>(s_part + (size_t)a.C * NW);
    float *s_scl = reinterpret_cast<float *>(s_list + (a.k < 0 ? 0 : min(a.k, deg)));
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];

    if (!rank && !emit) {
        // streaming row: add the tasks' partial rows in task order
        for (int c = tid; c < a.C; c += FIN_BLOCK) {
            float s = 0.f;
            for (int t = t0; t < t1; ++t) s += a.partial[(size_t)t * a.C + c];
            a.out_at<S>((size_t)i * a.C + c) = a.epilogue(s / (float)deg, i, c);
        }
        return;
    }

    const float *g_sc = a.scores + a.split_soff[p];
    const float *sc = g_sc;
    if (deg <= lds_scores) {
        for (int e = tid; e < deg; e += FIN_BLOCK) s_scl[e] = g_sc[e];
        sc = s_scl;
    }
    __syncthreads();

    int parity = 0;
    int c = 0;
    for (int e = tid; e < deg; e += FIN_BLOCK) c += (sc[e] >= a.thr);
    const int cnt_thr = block_count(c, sh, parity);
    unsigned long long T = 0;
    const bool thr_only = cnt_thr <= a.k;
    if (!thr_only) {
        int lowbits = 1;
        while ((1 << lowbits) < deg) ++lowbits;
        for (int b = 63; b >= 0; --b) {
            if (b == 31) { T |= ~((1ull << lowbits) - 1ull) & 0xFFFFFFFFull; b = lowbits - 1; }
            const unsigned long long cand = T | (1ull << b);
            c = 0;
            for (int e = tid; e < deg; e += FIN_BLOCK) c += (sel_key(sc[e], e) >= cand);
            if (block_count(c, sh, parity) >= a.k) T = cand;
        }
    }
    // ordered compaction of the kept edges (+ wsel)
    if (tid == 0) sh.nsel = 0;
    __syncthreads();
    for (int base = 0; base < deg; base += FIN_BLOCK) {
        const int e = base + tid;
        const float s = e < deg ? sc[e] : 0.f;
        const bool kept = e < deg && (thr_only ? (s >= a.thr) : (sel_key(s, e) >= T));
        const unsigned long long m = __ballot(kept);
        if (lane == 0) sh.wave_off[wave] = __popcll(m);
        __syncthreads();
        int off = sh.nsel;
        for (int w = 0; w < wave; ++w) off += sh.wave_off[w];
        if (kept) s_list[off + prefix_popc(m)] = e;
        if (rank && a.wsel && e < deg) a.wsel[rs + e] = kept ? s : SNGNN_UNSELECTED;
        __syncthreads();
        if (tid == 0) {
            int tot = 0;
            for (int w = 0; w < NW; ++w) tot += sh.wave_off[w];
            sh.nsel += tot;
        }
        __syncthreads();
    }
    const int nsel = sh.nsel;

    if (emit) {
        for (int q = tid; q < nsel; q += FIN_BLOCK) {
            const int idx = s_list[q];
            const unsigned long long kq = sel_key(sc[idx], idx);
            int rk = 0;
            for (int r = 0; r < nsel; ++r) {
                const int ir = s_list[r];
                rk += sel_key(sc[ir], ir) > kq;
            }
            a.sel_src[(size_t)i * a.k + rk] = a.col[rs + idx];
            a.sel_w[(size_t)i * a.k + rk] = sc[idx];
        }
    }

    RowT acc;
    acc.zero();
    if (rank) {
        for (int q0 = 0; q0 < nsel; q0 += NW * NG) {
            const int q = q0 + wave * NG + gid;
            if (q < nsel) {
                const int idx = s_list[q];
                const int j = a.col[rs + idx];
                RowT x;
                x.load(a.rows<S>() + (size_t)j * a.C, a.C, lg);
                acc.axpy(sc[idx] * (a.nrm ? a.nrm[j] : 1.0f), x);        // (OTF: the rows are h itself)
            }
        }
        acc.reduce_across_groups();
        if (gid == 0) acc.store(s_part + (size_t)wave * a.C, a.C, lg);
        __syncthreads();
        for (int ch = tid; ch < a.C; ch += FIN_BLOCK) {
            float s = 0.f;
            for (int w = 0; w < NW; ++w) s += s_part[(size_t)w * a.C + ch];
            a.out_at<S>((size_t)i * a.C + ch) = a.epilogue(s / (float)deg, i, ch);
        }
    } else {
        // emit on a streaming row: the sum itself still comes from the partials
        for (int ch = tid; ch < a.C; ch += FIN_BLOCK) {
            float s = 0.f;
            for (int t = t0; t < t1; ++t) s += a.partial[(size_t)t * a.C + ch];
            a.out_at<S>((size_t)i * a.C + ch) = a.epilogue(s / (float)deg, i, ch);
        }
    }
}

// ---------------------------------------------------------------------------
// Finalize of split rows from chunk-local candidates (top_k <= CAND_MAX_K):
// one 1024-thread workgroup per row merges the tasks' candidate keys 128 at a
// time (tournament of wave-level top-k) and gathers the <= k winners.
// ---------------------------------------------------------------------------
template <int VEC, int G, int R, int NW, bool HEAD, typename S = float>
__device__ __forceinline__ void fin_cand_row(const FwdArgs &a, int p, int max_slots, unsigned char *dyn)
{
    using RowT = Row<VEC, G, R>;
    constexpr int NG = 64 / G;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const int gid = lane / G, lg = lane % G;
    const int4 d = a.rdesc[p];
    const int i = d.x, rs = d.y, deg = d.z;
    if (a.skip_row(i)) return;                              // (workgroup-uniform)
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];
    const bool emit = a.sel_src != nullptr && a.k >= 0;
    const bool rank = a.k >= 0 && deg > a.k;

    // dynamic LDS: [FINC_WAVES_MAX * C] partial rows | keysA | keysB [max_slots] | srcA | srcB | count
    float *s_part = reinterpret_cast<float *>(dyn);
    unsigned long long *kA = reinterpret_cast<unsigned long long *>(s_part + (size_t)FINC_WAVES_MAX * a.C + ((FINC_WAVES_MAX * a.C) & 1));
    unsigned long long *kB = kA + max_slots;
    int *sA = reinterpret_cast<int *>(kB + max_slots);
    int *sB = sA + max_slots;
    int &s_n = sB[max_slots];

    if (!rank) {
        // streaming row (deg <= top_k or no selection): add the tasks' partial rows.  The
        // FINC_WAVES_MAX slices, slice s = the sum of every FINC_WAVES_MAX-th task from s on (a wave takes
        // the slices wave, wave + NW, ..: their loads in flight together), then the slices are added in
        // slice order: a fixed order WHATEVER the workgroup size, and a hub's ~100 partial
        // rows cost a handful of memory round trips instead of one each.
        for (int c0 = 0; c0 < a.C; c0 += 64) {
            const int c = c0 + lane;
            for (int sl = wave; sl < FINC_WAVES_MAX; sl += NW) {
                float s = 0.f;
                if (c < a.C)
                    for (int t = t0 + sl; t < t1; t += FINC_WAVES_MAX) s += a.partial[(size_t)t * a.C + c];
                if (c < a.C) s_part[(size_t)sl * a.C + c] = s;
            }
        }
        __syncthreads();
        for (int c = tid; c < a.C; c += (NW * 64)) {
            float s = 0.f;
            for (int w = 0; w < FINC_WAVES_MAX; ++w) s += s_part[(size_t)w * a.C + c];
            if constexpr (HEAD) s_part[c] = s / (float)deg;     // (C <= 64 <= (NW * 64): the thread's own channel only)
            else a.out_at<S>((size_t)i * a.C + c) = a.epilogue(s / (float)deg, i, c);
        }
        if constexpr (HEAD) {
            __syncthreads();
            fin_row_head<VEC, G, R>(a, i, p, s_part);
        }
        if (emit) {
            // selection of a streaming split row: every edge >= thr, ranked.  Rare
            // (needs top_k >= deg > WAVE_T); done by plain counting from the scratch scores.
            const float *sc = a.scores + a.split_soff[p];
            for (int e = tid; e < deg; e += (NW * 64)) {
                const float se = sc[e];
                if (!(se >= a.thr)) continue;
                int rk = 0;
                for (int b = 0; b < deg; ++b) rk += (sc[b] > se) || (sc[b] == se && b < e);
                a.sel_src[(size_t)i * a.k + rk] = a.col[rs + e];
                a.sel_w[(size_t)i * a.k + rk] = se;
            }
        }
        return;
    }

    int n = (t1 - t0) * a.k;
    for (int q = tid; q < n; q += (NW * 64)) {
        kA[q] = a.cand_key[(size_t)(t0 + q / a.k) * CAND_MAX_K + q % a.k];
        sA[q] = a.cand_src[(size_t)(t0 + q / a.k) * CAND_MAX_K + q % a.k];
    }
    __syncthreads();
    // tournament level: 256 keys per wave (4 per lane), so the biggest hub of an arxiv-like graph
    // (13 k in-edges: 102 tasks x 16 = 1 632 keys) is down to 7 x 16 = 112 keys - one wave-level
    // selection - after ONE level (128 per wave needed two levels and a third selection)
    while (n > 128) {
        const int groups = (n + 255) / 256;
        for (int g = wave; g < groups; g += NW) {
            unsigned long long key[4];
            int q[4];
            bool kp[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                q[u] = g * 256 + u * 64 + lane;
                key[u] = q[u] < n ? kA[q[u]] : 0ull;
            }
            wave_topk_keys_n<4, true>(key, a.k, a.lowbits, kp);
            int off = g * a.k;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned long long m = __ballot(kp[u]);
                if (kp[u]) { const int o = off + prefix_popc(m); kB[o] = key[u]; sB[o] = sA[q[u]]; }
                off += __popcll(m);
            }
            if (g * a.k + lane >= off && lane < a.k) kB[g * a.k + lane] = 0ull;      // empty slots (k <= 32 < 64)
        }
        __syncthreads();
        n = groups * a.k;
        unsigned long long *t = kA; kA = kB; kB = t;
        int *ts = sA; sA = sB; sB = ts;
    }
    if (wave == 0) {
        const unsigned long long key0 = lane < n ? kA[lane] : 0ull;
        const unsigned long long key1 = lane + 64 < n ? kA[lane + 64] : 0ull;
        bool k0, k1;
        wave_topk_cands(key0, key1, a.k, a.lowbits, k0, k1);
        const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1);
        const int n0 = __popcll(m0);
        if (k0) { const int o = prefix_popc(m0); kB[o] = key0; sB[o] = sA[lane]; }
        if (k1) { const int o = n0 + prefix_popc(m1); kB[o] = key1; sB[o] = sA[lane + 64]; }
        if (lane == 0) s_n = n0 + __popcll(m1);
    }
    __syncthreads();
    const int nsel = s_n;
    const unsigned long long *win = kB;
    const int *wsrc = sB;

    // gather first (the long latency), bookkeeping stores behind it
    RowT acc;
    acc.zero();
    for (int q0 = 0; q0 < nsel; q0 += NW * NG) {
        const int q = q0 + wave * NG + gid;
        if (q < nsel) {
            const int j = wsrc[q];
            RowT x;
            x.load(a.rows<S>() + (size_t)j * a.C, a.C, lg);
            acc.axpy(key_score(win[q]) * (a.nrm ? a.nrm[j] : 1.0f), x);
        }
    }
    for (int q = tid; q < nsel; q += (NW * 64)) {
        const unsigned long long kq = win[q];
        const float sq = key_score(kq);
        if (a.wsel) a.wsel[rs + key_index(kq)] = sq;
        if (a.kbits) atomicOr(a.kbits + a.kb_tbase + 4 * t0 + (key_index(kq) >> 5), 1u << (key_index(kq) & 31));
        if (emit) {
            int rk = 0;
            for (int r = 0; r < nsel; ++r) rk += win[r] > kq;
            a.sel_src[(size_t)i * a.k + rk] = wsrc[q];
            a.sel_w[(size_t)i * a.k + rk] = sq;
        }
    }
    acc.reduce_across_groups();
    if (gid == 0) acc.store(s_part + (size_t)wave * a.C, a.C, lg);
    __syncthreads();
    for (int ch = tid; ch < a.C; ch += (NW * 64)) {
        float s = 0.f;
        for (int w = 0; w < NW; ++w) s += s_part[(size_t)w * a.C + ch];
        if constexpr (HEAD) s_part[ch] = s / (float)deg;
        else a.out_at<S>((size_t)i * a.C + ch) = a.epilogue(s / (float)deg, i, ch);
    }
    if constexpr (HEAD) {
        __syncthreads();
        fin_row_head<VEC, G, R>(a, i, p, s_part);
    }
}

template <int VEC, int G, int R, int NW, bool HEAD, typename S = float>
__global__ __launch_bounds__(NW * 64) void k_agg_fin_cand(const FwdArgs a, int max_slots)
{
    extern __shared__ __align__(16) unsigned char dyn[];   // no static LDS in front of it
    fin_cand_row<VEC, G, R, NW, HEAD, S>(a, blockIdx.x, max_slots, dyn);
}

// The same finalize for split rows whose candidates fit one wave-level selection
// ((tasks) * k <= 128, i.e. deg <= 8 * CHUNK at k = 16): one WAVE per row, no workgroup
// barrier.  On graphs with many moderately large rows
// (products-like: ~10^5 split rows) the 1024-thread tournament (fin_cand_row) is mostly idle.
// s_key_w / s_src_w: the wave's own CAND_MAX_K LDS slots.
template <int VEC, int G, int R, bool HEAD, typename S = float>
__device__ __forceinline__ void fin_wave_row(const FwdArgs &a, int p, unsigned long long *s_key_w, int *s_src_w)
{
    using RowT = Row<VEC, G, R>;
    const int lane = lane_id();
    const int gid = lane / G, lg = lane % G;
    const int4 d = a.rdesc[p];
    const int i = d.x, rs = d.y, deg = d.z;
    if (a.skip_row(i)) return;                              // (wave-uniform)
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];
    int head_yy = 0;
    unsigned head_sv = 0u;
    if constexpr (HEAD) { head_yy = (int)a.head_y[i]; head_sv = a.head_sel[i]; }
    if (a.k < 0) {
        // (rows of at most 16 tasks come here: their partial rows are loaded together)
        float *s_row = reinterpret_cast<float *>(s_key_w);      // head: the row through LDS (C <= 64 floats fit)
        for (int c = lane; c < a.C; c += 64) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = t0 + u < t1 ? a.partial[(size_t)(t0 + u) * a.C + c] : 0.f;
            float s = 0.f;
#pragma unroll
            for (int u = 0; u < 16; ++u) s += v[u];
            for (int t = t0 + 16; t < t1; ++t) s += a.partial[(size_t)t * a.C + c];
            if constexpr (HEAD) s_row[c] = s / (float)deg;
            else a.out_at<S>((size_t)i * a.C + c) = a.epilogue(s / (float)deg, i, c);
        }
        if constexpr (HEAD) {
            if constexpr (VEC == 4 && R == 1 && (G == 8 || G == 16)) {
                wave_lds_sync();
                HeadAcc ha;
                if (gid == 0) {
                    RowT row;
                    const float4 t = *reinterpret_cast<const float4 *>(s_row + (4 * lg < a.C ? 4 * lg : 0));
                    row.x[0][0] = t.x; row.x[0][1] = t.y; row.x[0][2] = t.z; row.x[0][3] = t.w;
                    head_store_row<VEC, G, R>(a, row, i, lg, head_yy, head_sv, ha);
                }
                head_write_entry(a, a.head_nmain + p, ha);
            }
        }
        return;
    }
    const int n = (t1 - t0) * a.k;                            // <= 128 by the launch split
    auto slot = [&](int q) { return (size_t)(t0 + q / a.k) * CAND_MAX_K + q % a.k; };
    const unsigned long long key0 = lane < n ? a.cand_key[slot(lane)] : 0ull;
    const unsigned long long key1 = lane + 64 < n ? a.cand_key[slot(lane + 64)] : 0ull;
    const int src0 = lane < n ? a.cand_src[slot(lane)] : 0;
    const int src1 = lane + 64 < n ? a.cand_src[slot(lane + 64)] : 0;
    bool k0, k1;
    wave_topk_cands(key0, key1, a.k, a.lowbits, k0, k1);
    const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1);
    const int n0 = __popcll(m0), nsel = n0 + __popcll(m1);
    if (k0) { const int o = prefix_popc(m0); s_key_w[o] = key0; s_src_w[o] = src0; }
    if (k1) { const int o = n0 + prefix_popc(m1); s_key_w[o] = key1; s_src_w[o] = src1; }
    wave_lds_sync();
    fin_winners_row<VEC, G, R, HEAD, S>(a, p, i, rs, deg, t0, nsel, s_key_w, s_src_w, head_yy, head_sv);
}

// 4 rows per 256-thread workgroup
template <int VEC, int G, int R, bool HEAD, typename S = float>
__global__ __launch_bounds__(BLOCK) void k_agg_fin_wave(const FwdArgs a, int first, int count)
{
    __shared__ unsigned long long s_key[WAVES][CAND_MAX_K];
    __shared__ int s_src[WAVES][CAND_MAX_K];
    const int wave = threadIdx.x >> 6;
    const int q = blockIdx.x * WAVES + wave;
    if (q >= count) return;                                   // wave-uniform
    fin_wave_row<VEC, G, R, HEAD, S>(a, first + q, s_key[wave], s_src[wave]);
}
// Both in ONE launch when the moderate split rows are few (arxiv-like graphs: a few hundred
// split rows in all): workgroups [0, n_big) run the tournament of one big row each, the
// others one moderate row per wave - 140 workgroups that all start at once instead of 825
// tournaments of which 512 fit the chip (finalize 8.8 -> see DESIGN.md 4.1).
// HEAD: its own instantiation (the head's code inside the plain one cost it 9 registers, 12 bytes of
// scratch per lane and ~0.5 us of the headline step)
template <int VEC, int G, int R, int NW, bool HEAD, typename S = float>
__global__ __launch_bounds__(NW * 64) void k_agg_fin_mixed(const FwdArgs a, int max_slots, int n_big, int n_split,
                                                              int n_fin_blocks)
{
    extern __shared__ __align__(16) unsigned char dyn[];   // no static LDS in front of it
    if constexpr (HEAD) {
        if ((int)blockIdx.x >= n_fin_blocks) {             // (workgroup-uniform) the head role of the launch
            const int hb = (int)blockIdx.x - n_fin_blocks;
            const HeadAcc ha = head_rows_role<VEC, G, R>(a, hb * NW + (threadIdx.x >> 6), a.head_nmain * NW);
            head_block_entry(a, hb, ha, reinterpret_cast<float *>(dyn));
            return;
        }
    }
    if ((int)blockIdx.x < n_big) {                         // (workgroup-uniform)
        fin_cand_row<VEC, G, R, NW, HEAD, S>(a, blockIdx.x, max_slots, dyn);
        return;
    }
    const int wave = threadIdx.x >> 6;
    const int p = n_big + ((int)blockIdx.x - n_big) * NW + wave;
    if (p >= n_split) return;                              // wave-uniform
    unsigned long long *s_key = reinterpret_cast<unsigned long long *>(dyn) + wave * CAND_MAX_K;
    int *s_src = reinterpret_cast<int *>(dyn + NW * CAND_MAX_K * 8) + wave * CAND_MAX_K;
    fin_wave_row<VEC, G, R, HEAD, S>(a, p, s_key, s_src);
}

}  // namespace sngnn
