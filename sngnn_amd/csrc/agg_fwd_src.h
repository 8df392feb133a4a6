// How the forward's work-item roles read their gathered inputs - table rows, norms, column ids, the small rows'
// descriptors, fp16 filter rows - in two forms behind one interface (agg_fwd_roles.h takes it as `src`):
//   FwdSrc<false, ..>  FLAT: 64-bit pointers.  A slot nobody reads (beyond the row's edges, beyond the list) loads the
//       row's own feature row `self` instead - an address that is valid and cache-hot - and lanes beyond C load
//       channel 0 and zero it afterwards (Row::load).  The form for tables of 2 GiB and more, and the A/B reference.
//   FwdSrc<true, ..>   BUFFER (buffer_addr.h): one resource per array, built once per kernel from FwdArgs, and a 32-bit
//       byte offset per load: row j's is j * 4C (one 32-bit multiply) plus the lane's own term, which is computed once
//       per kernel - the lane's channel offset, or BUF_OOB for a lane beyond C.  A slot nobody reads gets BUF_OOB for
//       the row: the load returns zeros and sends no request, where the flat form loads `self` and runs on it.
// The values loaded for every slot that IS read are the same bits in both forms, and the arithmetic behind the loads
// is shared: results are bit-identical (tests/test_fwd_buffer_addr_gpu.py).  fp32 tables only: the half path's rows
// (S = __half / __hip_bfloat16) keep the flat form.
#pragma once
#include "agg_fwd_args.h"

namespace sngnn {

template <bool BUF, int VEC, int G, int R, typename S> struct FwdSrc;

template <int VEC, int G, int R, typename S> struct FwdSrc<false, VEC, G, R, S> {
    using RowT = Row<VEC, G, R>;
    static constexpr bool skips_dead = false;     // every slot of a small-row set is loaded and scored
    const FwdArgs &a;
    int lg;
    __device__ __forceinline__ FwdSrc(const FwdArgs &a_, int lg_) : a(a_), lg(lg_) {}
    // the id a dead slot gathers: the flat form needs a valid one
    __device__ __forceinline__ int pick(bool live, int j, int self) const { return live ? j : self; }
    __device__ __forceinline__ void row(RowT &x, int j) const { x.load(a.rows<S>() + (size_t)j * a.C, a.C, lg); }
    // (j = pick(..) or a col_if() value: valid whether the slot is live or not)
    __device__ __forceinline__ void row_if(RowT &x, int j, bool) const { row(x, j); }
    __device__ __forceinline__ float nrm(int j) const { return a.nrm[j]; }
    __device__ __forceinline__ float nrm_if(int j, bool) const { return a.nrm[j]; }
    // the norm unless the caller has no use for it (`skip`: then 0)
    __device__ __forceinline__ float nrm_unless(int j, bool, bool skip) const { return skip ? 0.f : a.nrm[j]; }
    __device__ __forceinline__ int col_if(int e, bool live, int self) const { return live ? a.col[e] : self; }
    __device__ __forceinline__ int col_s_if(int e, bool live) const { return live ? a.col_s[e] : 0; }
    __device__ __forceinline__ int4 desc_if(int slot, bool live) const
    {
        return live ? a.rdesc[slot] : make_int4(0, 0, 0, -1);
    }
    // entry `idx` (0 .. 8 G R / W) of node j's filter row, in units of W = sizeof(T) bytes
    template <typename T> __device__ __forceinline__ T filt(int j, int per_row, int idx) const
    {
        return reinterpret_cast<const T *>(a.filt)[(size_t)j * per_row + idx];
    }
    template <typename T> __device__ __forceinline__ T filt_if(int j, bool, int per_row, int idx) const
    {
        return filt<T>(j, per_row, idx);
    }
};

template <int VEC, int G, int R> struct FwdSrc<true, VEC, G, R, float> {
    using RowT = Row<VEC, G, R>;
    // a small-row set skips the slots beyond its longest row (small_rows_set)
    static constexpr bool skips_dead = true;
    __amdgpu_buffer_rsrc_t r_n, r_nrm, r_col, r_col_s, r_desc, r_filt;
    unsigned row_bytes;
    unsigned loff[R];          // the lane's term of a row offset, per step: its channels' byte offset, or BUF_OOB
    __device__ __forceinline__ FwdSrc(const FwdArgs &a, int lg)
    {
        r_n = make_rsrc(a.n, a.n_bytes);
        r_nrm = make_rsrc(a.nrm, a.nrm != nullptr ? (unsigned)a.Ntot * 4u : 0u);
        // (the launcher's rule, fwd_plan.h: 4 E' < 2^31 as well)
        r_col = make_rsrc(a.col, (unsigned)a.n_edges * 4u);
        r_col_s = make_rsrc(a.col_s, (unsigned)a.n_edges * 4u);
        r_desc = make_rsrc(a.rdesc, (unsigned)a.N * 16u);
        r_filt = make_rsrc(a.filt, a.filt != nullptr ? (unsigned)a.Ntot * (unsigned)(8 * G * R) : 0u);
        row_bytes = (unsigned)a.C * 4u;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int c0 = (r * G + lg) * VEC;
            loff[r] = c0 < a.C ? (unsigned)c0 * 4u : BUF_OOB;
        }
    }
    __device__ __forceinline__ int pick(bool, int j, int) const { return j; }
    __device__ __forceinline__ void row(RowT &x, int j) const
    {
        const unsigned ro = (unsigned)j * row_bytes;
        unsigned off[R];
#pragma unroll
        for (int r = 0; r < R; ++r) off[r] = ro + loff[r];
        x.load_buf(r_n, off);
    }
    __device__ __forceinline__ void row_if(RowT &x, int j, bool live) const
    {
        const unsigned ro = live ? (unsigned)j * row_bytes : BUF_OOB;
        unsigned off[R];
#pragma unroll
        for (int r = 0; r < R; ++r) off[r] = buf_off_add_sat(ro, loff[r]);
        x.load_buf(r_n, off);
    }
    __device__ __forceinline__ float nrm(int j) const
    {
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r_nrm, (unsigned)j * 4u, 0, 0));
    }
    __device__ __forceinline__ float nrm_if(int j, bool live) const
    {
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r_nrm, live ? (unsigned)j * 4u : BUF_OOB, 0, 0));
    }
    // (`skip` differs between the lane groups of a small-row set: the load is issued, with a dead offset)
    __device__ __forceinline__ float nrm_unless(int j, bool live, bool skip) const { return nrm_if(j, live && !skip); }
    // (a dead slot's id is 0 and is never a row's address: row_if / nrm_if take the same `live`)
    __device__ __forceinline__ int col_if(int e, bool live, int) const
    {
        return (int)__builtin_amdgcn_raw_buffer_load_b32(r_col, live ? (unsigned)e * 4u : BUF_OOB, 0, 0);
    }
    __device__ __forceinline__ int col_s_if(int e, bool live) const
    {
        return (int)__builtin_amdgcn_raw_buffer_load_b32(r_col_s, live ? (unsigned)e * 4u : BUF_OOB, 0, 0);
    }
    __device__ __forceinline__ int4 desc_if(int slot, bool live) const
    {
        const auto t = __builtin_amdgcn_raw_buffer_load_b128(r_desc, live ? (unsigned)slot * 16u : BUF_OOB, 0, 0);
        return make_int4((int)t[0], (int)t[1], (int)t[2], live ? (int)t[3] : -1);
    }
    template <typename T> __device__ __forceinline__ T filt_at(unsigned off) const
    {
        static_assert(sizeof(T) == 8 || sizeof(T) == 16, "filter rows are read 8 or 16 bytes per lane");
        if constexpr (sizeof(T) == 16) {
            const auto t = __builtin_amdgcn_raw_buffer_load_b128(r_filt, off, 0, 0);
            return make_uint4(t[0], t[1], t[2], t[3]);
        } else {
            const auto t = __builtin_amdgcn_raw_buffer_load_b64(r_filt, off, 0, 0);
            return make_uint2(t[0], t[1]);
        }
    }
    template <typename T> __device__ __forceinline__ T filt(int j, int per_row, int idx) const
    {
        return filt_at<T>(((unsigned)j * (unsigned)per_row + (unsigned)idx) * (unsigned)sizeof(T));
    }
    template <typename T> __device__ __forceinline__ T filt_if(int j, bool live, int per_row, int idx) const
    {
        return filt_at<T>(live ? ((unsigned)j * (unsigned)per_row + (unsigned)idx) * (unsigned)sizeof(T) : BUF_OOB);
    }
};

}  // namespace sngnn
