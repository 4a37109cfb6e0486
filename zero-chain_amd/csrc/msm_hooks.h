// Test hooks of the table multiples (msm_types.h MsmRecode; tests/test_table_multiples.py): the recoding of single scalars, a group
// built with multiples - its table entries and launch sets over it - and what ensure_derived bound.  Included by zkamd.cpp
// under -DZK_TEST_HOOKS only; the multiples and the extra window bits are run-time arguments here.
#pragma once
#ifdef ZK_TEST_HOOKS
#include "msm_recode.h"

namespace zkdev {

// the digits of n scalars through msm_digits, four words each: position, odd bucket magnitude, multiple index, negative
static __global__ void __launch_bounds__(64)
k_hook_recode(const uint32_t* __restrict__ scalars, uint32_t n, uint32_t c, const MsmRecode rc, uint32_t cap, uint32_t* out, uint32_t* count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const MsmJob job = {scalars, nullptr, n, 0u, 0u, 0u, 0u, 0u};
    uint32_t k = 0;
    msm_digits(job, i, c, rc, [&](uint32_t slot, uint32_t slice, uint32_t mag, bool negative) {
        if (slot < cap) {
            uint32_t* o = out + ((size_t)i * cap + slot) * 4;
            o[0] = slice % MSM_NPOS;
            o[1] = mag;
            o[2] = slice / MSM_NPOS;
            o[3] = negative ? 1u : 0u;
        }
        k = slot + 1;
    });
    count[i] = k;
}

// out[t] = entry idx[t] of a table as a point
template <class F>
static __global__ void __launch_bounds__(64)
k_hook_table_entries(const Affine<F>* __restrict__ table, const uint32_t* __restrict__ idx, uint32_t n, XYZZ<F>* out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = XYZZ<F>::from_affine(table[idx[t]]);
}

}  // namespace zkdev

namespace {

template <class F>
F hook_field_of(const zkdev::Affine<F>*);

inline bool hook_mult_args(uint32_t c, uint32_t n_mult, uint32_t ext) {
    return c >= 3 && n_mult >= 1 && n_mult <= zkdev::MSM_MULT_MAX && ext <= 7 && c + ext <= 22 && (n_mult > 1 || ext == 0);
}

// A group over n_bases encoded points with n_mult multiples per slice (extra window bits ext), then - in this order - the table
// entries (multiple, slice, base) asked for and n_jobs jobs of n scalars through one map (msm_types.h MsmSelRange over them as in
// zk_hook_msm_select).  A base that is the identity is mapped out, as the key's decoder does it.
template <class Group, class HA, class HP, class Dec, class Enc>
zk_status hook_mult_msm(Dec&& decode, Enc&& encode, size_t enc_bytes, uint32_t c, uint32_t n_mult, uint32_t ext, uint32_t n_bases, const uint8_t* bases,
                        uint32_t n_jobs, uint32_t n, const uint8_t* scalars, const int32_t* map, const uint8_t* sel, const int32_t* alt,
                        uint32_t sel_first, uint32_t sel_n, uint32_t alt_w, uint8_t* out, uint32_t n_entries, const uint32_t* entries,
                        uint8_t* entries_out) {
    typedef typename Group::DAffine DA;
    typedef typename Group::DPoint DP;
    typedef decltype(hook_field_of((const DA*)nullptr)) DF;
    if (!hook_mult_args(c, n_mult, ext) || !n_bases || !bases) return fail(ZK_ERR_INVALID_ARGUMENT, "width, multiples or bases out of range");
    if (n_jobs && (!n || !scalars || !map || !out)) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (sel && (!alt || (size_t)sel_first + sel_n > n || alt_w > 6)) return fail(ZK_ERR_INVALID_ARGUMENT, "the bytes do not fit the job");
    std::vector<HA> pts(n_bases);
    for (uint32_t i = 0; i < n_bases; i++)
        if (decode(bases + (size_t)i * enc_bytes, &pts[i]) != zkhost::DEC_OK) return fail(ZK_ERR_IO, "a base does not decode");
    ZK_TRY(use_device(g_device < 0 ? 0 : g_device));
    Group g;
    ZK_TRY(g.build(pts, c, false, "hook bases", true, n_mult));
    if (n_mult > 1 && ext != g.ext) {   // (build made the choice table of the default extra bits)
        g.ext = ext;
        g.lut.release();
    }
    if (n_entries) {
        if (!entries || !entries_out) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
        std::vector<uint32_t> idx(n_entries);
        for (uint32_t t = 0; t < n_entries; t++) {
            const uint32_t j = entries[3 * t], k = entries[3 * t + 1], i = entries[3 * t + 2];
            if (j >= n_mult || k >= zkdev::MSM_NPOS || i >= n_bases) return fail(ZK_ERR_INVALID_ARGUMENT, "table entry out of range");
            idx[t] = (j * zkdev::MSM_NPOS + k) * n_bases + i;
        }
        DevBuf d_idx, d_pts, stage;
        ZK_TRY(d_idx.upload(idx));
        ZK_TRY(d_pts.ensure((size_t)n_entries * sizeof(DP)));
        ZK_LAUNCH(zkdev::k_hook_table_entries<DF>, dim3((n_entries + 63) / 64), dim3(64), 0, g_stream, (const DA*)g.table.template as<DA>(),
                  (const uint32_t*)d_idx.as<uint32_t>(), n_entries, d_pts.as<DP>());
        HIP_TRY(hipGetLastError());
        std::vector<HP> host(n_entries);
        ZK_TRY(g.export_to_host(d_pts.as<DP>(), n_entries, host.data(), stage, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));
        for (uint32_t t = 0; t < n_entries; t++) encode(zkhost::to_affine(host[t]), entries_out + (size_t)t * enc_bytes);
    }
    if (!n_jobs) return ZK_OK;
    std::vector<int32_t> mp(map, map + n);
    for (uint32_t i = 0; i < n; i++) {
        if (mp[i] < -1 || mp[i] >= (int32_t)n_bases) return fail(ZK_ERR_INVALID_ARGUMENT, "map out of range");
        if (mp[i] >= 0 && pts[mp[i]].is_inf()) mp[i] = -1;
    }
    std::vector<int32_t> al(alt ? (size_t)sel_n * alt_w : 0);
    for (size_t i = 0; i < al.size(); i++) {
        al[i] = alt[i];
        if (al[i] < -1 || al[i] >= (int32_t)n_bases) return fail(ZK_ERR_INVALID_ARGUMENT, "alternate out of range");
        if (al[i] >= 0 && pts[al[i]].is_inf()) al[i] = -1;
    }
    DevBuf d_sc, d_map, d_sel, d_alt;
    ZK_TRY(d_sc.ensure((size_t)n_jobs * n * 32));
    HIP_TRY(hipMemcpy(d_sc.p, scalars, (size_t)n_jobs * n * 32, hipMemcpyHostToDevice));
    ZK_TRY(d_map.upload(mp));
    if (sel) {
        ZK_TRY(d_sel.ensure((size_t)n_jobs * sel_n + 1));
        ZK_TRY(d_alt.ensure(al.size() * 4 + 4));
        HIP_TRY(hipMemcpy(d_sel.p, sel, (size_t)n_jobs * sel_n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_alt.p, al.data(), al.size() * 4, hipMemcpyHostToDevice));
    }
    std::vector<MsmJob> jobs;
    for (uint32_t p = 0; p < n_jobs; p++) {
        MsmJob j = {d_sc.as<uint32_t>() + (size_t)p * n * 8, d_map.as<int32_t>(), n, 0u, n_bases, 0, 0, 0};
        jobs.push_back(j);
    }
    zkdev::MsmSelSet sels = {};
    if (sel) sels.r[0] = {d_sel.as<uint8_t>(), d_alt.as<int32_t>(), 0u, n_jobs, sel_n, sel_first, sel_n, alt_w};
    std::vector<HP> res;
    ZK_TRY(g.run(jobs, res, &sels));
    for (uint32_t p = 0; p < n_jobs; p++) encode(zkhost::to_affine(res[p]), out + (size_t)p * enc_bytes);
    return ZK_OK;
}

}  // namespace

extern "C" {

// Test hook: the recoding of n scalars (plain words) at width c over n_mult multiples with ext extra window bits; out: cap x 4
// words per scalar (position, bucket magnitude, multiple index, negative), count: digits per scalar (may exceed cap)
zk_status zk_hook_recode(uint32_t c, uint32_t n_mult, uint32_t ext, uint32_t n, const uint8_t* scalars, uint32_t cap, uint32_t* out,
                         uint32_t* count) try {
    if (!hook_mult_args(c, n_mult, ext) || !n || !scalars || !cap || !out || !count) return fail(ZK_ERR_INVALID_ARGUMENT, "argument out of range");
    ZK_TRY(use_device(g_device < 0 ? 0 : g_device));
    DevBuf d_sc, d_out, d_cnt, d_lut;
    ZK_TRY(d_sc.ensure((size_t)n * 32));
    HIP_TRY(hipMemcpy(d_sc.p, scalars, (size_t)n * 32, hipMemcpyHostToDevice));
    ZK_TRY(d_out.ensure((size_t)n * cap * 16));
    ZK_TRY(d_cnt.ensure((size_t)n * 4));
    HIP_TRY(hipMemset(d_out.p, 0xff, (size_t)n * cap * 16));
    if (n_mult > 1) {
        std::vector<uint8_t> h((size_t)1 << (c + ext - 1));
        for (size_t v = 0; v < h.size(); v++) h[v] = zkdev::msm_mult_choice((uint32_t)(2 * v + 1), c, n_mult, ext);
        ZK_TRY(d_lut.upload(h));
    }
    const zkdev::MsmRecode rc = {d_lut.as<uint8_t>(), n_mult, ext};
    ZK_LAUNCH(zkdev::k_hook_recode, dim3((n + 63) / 64), dim3(64), 0, g_stream, (const uint32_t*)d_sc.as<uint32_t>(), n, c, rc, cap,
              d_out.as<uint32_t>(), d_cnt.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));
    HIP_TRY(hipMemcpy(out, d_out.p, (size_t)n * cap * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(count, d_cnt.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return ZK_OK;
} ZK_ABI_CATCH

// Test hook: a group (1: G1, 2: G2) over encoded bases with multiples - see hook_mult_msm.  entries: n_entries x (multiple
// index, slice, base); entries_out / out: uncompressed points.
zk_status zk_hook_mult_msm(int group, uint32_t c, uint32_t n_mult, uint32_t ext, uint32_t n_bases, const uint8_t* bases, uint32_t n_jobs,
                           uint32_t n, const uint8_t* scalars, const int32_t* map, const uint8_t* sel, const int32_t* alt, uint32_t sel_first,
                           uint32_t sel_n, uint32_t alt_w, uint8_t* out, uint32_t n_entries, const uint32_t* entries, uint8_t* entries_out) try {
    if (group == 1)
        return hook_mult_msm<MsmG1, HG1A, HG1>(zkhost::g1_from_uncompressed, zkhost::g1_to_uncompressed, 96, c, n_mult, ext, n_bases, bases, n_jobs, n,
                                               scalars, map, sel, alt, sel_first, sel_n, alt_w, out, n_entries, entries, entries_out);
    if (group == 2)
        return hook_mult_msm<MsmG2, HG2A, HG2>(zkhost::g2_from_uncompressed, zkhost::g2_to_uncompressed, 192, c, n_mult, ext, n_bases, bases, n_jobs, n,
                                               scalars, map, sel, alt, sel_first, sel_n, alt_w, out, n_entries, entries, entries_out);
    return fail(ZK_ERR_INVALID_ARGUMENT, "group must be 1 or 2");
} ZK_ABI_CATCH

// Test hook: what ensure_derived bound for the key: info = [multiples of the G1 table, of the G2 table, C' width, A width, G2 width,
// choice-table bits of the C' set]
zk_status zk_hook_bound_multiples(const zk_params* p, uint32_t info[6]) try {
    if (!p || !info) return fail(ZK_ERR_INVALID_ARGUMENT, "null argument");
    if (!p->bind.drv.ready) return fail(ZK_ERR_INVALID_ARGUMENT, "the key is bound to no circuit");
    const uint32_t f[6] = {p->bind.g1d.n_mult, p->bind.g2p.n_mult, p->bind.g1d.c, p->bind.g1da.c, p->bind.g2p.c, p->bind.g1d.c + p->bind.g1d.ext};
    std::copy(f, f + 6, info);
    return ZK_OK;
} ZK_ABI_CATCH

}  // extern "C"
#endif
