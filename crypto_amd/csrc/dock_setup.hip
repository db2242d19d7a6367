// crypto_amd/csrc/dock_setup.hip — LegoGroth16 key generation from a resident circuit (include/dock_gpu.h: dgpu_qap_instance_map,
// dgpu_legogroth16_setup).  Replaces generate_parameters_and_extra_info_with_qap (/root/reference/legogroth16/src/generator.rs:245-442) with
// LibsnarkReduction::instance_map_with_evaluation (r1cs_to_qap.rs:105-147) and the h scalars (r1cs_to_qap.rs:212-223) in front of it.
// The scalar half runs on the device (setup_kernels.hip.h); the O(1) field constants (Z(t), 1/gamma, 1/delta, ...) are computed here on the host.
// Every FixedBase::msm is a window-table product from the scalars where they were computed: nothing per element crosses PCIe.
#include "msm_driver.hip.h"
#include "fixed_launch.hip.h"
#include "setup_launch.hip.h"

namespace dock {
template <class C> int32_t table_mul_device(Slot &sl, const void *table, const uint32_t *d_scalars, size_t n, void **keep, uint64_t *out, uint8_t *out_inf);   // dock_fixed.hip
}
using namespace dock;
using hostf::FrH;

namespace {

constexpr size_t FRB = ntt::FR_WORDS * 4;       // bytes per internal Fr element

// 4 words -> field element: canonical (any value below 2^256, reduced) or ark-ff Montgomery limbs
FrH fr_in(const uint64_t w[4], bool mont) {
    FrH a, r2, one{{1, 0, 0, 0}}; memcpy(a.l, w, 32); memcpy(r2.l, FrH::R2, 32);
    FrH x = a * r2;                               // Montgomery form of the value w
    return mont ? x * one : x;                    // (Montgomery words: the value w / 2^256, whose Montgomery form is w mod r)
}
void fr_out(const FrH &x, bool mont, uint64_t out[4]) { if (mont) memcpy(out, x.l, 32); else x.to_canonical(out); }
bool fr_is_zero(const FrH &x) { return (x.l[0] | x.l[1] | x.l[2] | x.l[3]) == 0; }

// one device block for the whole call, freed (after the stream has drained) on every return path
struct Block {
    void *p = nullptr; hipStream_t s = nullptr;
    ~Block() { if (p) { (void)hipStreamSynchronize(s); (void)hipFree(p); } }
};
struct Carve {
    uint8_t *base; size_t off = 0;
    template <class T> T *take(size_t bytes) { T *r = (T *)(base + off); off += (bytes + 255) & ~(size_t)255; return r; }
};

struct Domain { int logn; size_t D; FrH zt, omega; };
int32_t domain_for(const R1csView &r, const FrH &t, Domain &d) {
    d.logn = 0;
    while (((size_t)1 << d.logn) < r.num_constraints + r.num_inputs) d.logn++;       // ark-poly Radix2EvaluationDomain::new (no minimum of 2)
    if (d.logn > 28) return DGPU_E_BADARG;
    d.D = (size_t)1 << d.logn;
    const uint64_t e[4] = {d.D, 0, 0, 0};
    d.zt = t.pow(e).sub_one();
    if (fr_is_zero(d.zt)) return DGPU_E_BADARG;     // t in the domain: every u_i has a zero denominator
    d.omega = FrH::root_of_unity(d.logn);
    return DGPU_OK;
}
size_t im_bytes(const R1csView &r, size_t D, const size_t nnz[3]) {
    size_t scratch = 0;
    for (int k = 0; k < 3; k++) scratch = std::max(scratch, setupk::col_sum_scratch_bytes(nnz[k], r.num_vars));
    return 2 * (D * FRB + 256) + 3 * (r.num_vars * FRB + 256) + scratch + 256 + 4 * 256;
}
// the nnz of each matrix: rowptr[rows] (the upload keeps one placeholder entry for an empty matrix)
int32_t real_nnz(Slot &sl, const R1csView &r, size_t nnz[3]) {
    uint64_t v[3];
    for (int k = 0; k < 3; k++) HIPCHK(hipMemcpyAsync(&v[k], r.rowptr[k] + r.num_constraints, 8, hipMemcpyDeviceToHost, sl.stream));
    HIPCHK(hipStreamSynchronize(sl.stream));
    for (int k = 0; k < 3; k++) { nnz[k] = v[k]; if (v[k] > r.vstride[k] || v[k] >= (1ull << 32)) return DGPU_E_BADARG; }
    return DGPU_OK;
}
// instance_map_with_evaluation: a, b, c (SoA, stride num_vars) from t.  pw is left free for the caller (D elements).
struct ImOut { uint32_t *a, *b, *c, *pw, *consts; };
int32_t instance_map_device(Slot &sl, const R1csView &r, const FrH &t, const Domain &d, const size_t nnz[3], Carve &cv, ImOut &o) {
    hipStream_t s = sl.stream;
    const size_t nv = r.num_vars, D = d.D;
    o.pw = cv.take<uint32_t>(D * FRB);
    uint32_t *u = cv.take<uint32_t>(D * FRB);
    o.a = cv.take<uint32_t>(nv * FRB); o.b = cv.take<uint32_t>(nv * FRB); o.c = cv.take<uint32_t>(nv * FRB);
    o.consts = cv.take<uint32_t>(1024);
    size_t scratch_bytes = 0;
    for (int k = 0; k < 3; k++) scratch_bytes = std::max(scratch_bytes, setupk::col_sum_scratch_bytes(nnz[k], nv));
    void *scratch = cv.take<void>(scratch_bytes);
    // consts: [omega, 1, t, Z(t) / D] as canonical words
    uint64_t cw[4][4];
    const FrH dinv = FrH::from_u64(D).inv();
    d.omega.to_canonical(cw[0]); FrH::from_u64(1).to_canonical(cw[1]); t.to_canonical(cw[2]); (d.zt * dinv).to_canonical(cw[3]);
    HIPCHK(hipMemcpyAsync(o.consts, cw, sizeof cw, hipMemcpyHostToDevice, s));
    StageTimer st(sl, "setup.instance_map");
    ntt::launch_fr_powers(s, o.consts + 0, o.consts + 8, D, o.pw);                     // w^i
    setupk::launch_lagrange(s, o.pw, o.consts + 16, D, u);                              // u_i
    setupk::launch_im_init(s, u, D, r.num_constraints, r.num_inputs, nv, o.a, o.b, o.c);
    uint32_t *outs[3] = {o.a, o.b, o.c};
    for (int k = 0; k < 3; k++)
        setupk::launch_col_sum(s, r.rowptr[k], r.num_constraints, r.cols[k], r.vals[k], r.vstride[k], nnz[k], u, D, outs[k], nv, scratch);
    if (hipGetLastError() != hipSuccess) return DGPU_E_HIP;
    return DGPU_OK;
}

struct Keep {          // bases allocations not yet registered: freed unless the call succeeds
    void *p[5] = {};
    ~Keep() { for (void *q : p) if (q) (void)hipFree(q); }
};

struct SetupOut { uint64_t *handles, *g1, *g2, *gamma_abc; size_t gamma_abc_cap; uint64_t *xy[5]; uint8_t *inf[5]; size_t *domain_size; };
int32_t setup(uint64_t r1cs, size_t cw, const uint64_t *w, const uint64_t *g1, const uint64_t *g2, int32_t montgomery, SetupOut &o) {
    if (!w || !g1 || !g2 || !o.handles || !o.g1 || !o.g2) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    HandleRef href(r1cs);
    if (!href.ok || href.h.kind != 4) return DGPU_E_BADARG;
    const R1csView r = r1cs_view(href.h.p);
    const bool mont = montgomery != 0;
    const FrH alpha = fr_in(w, mont), beta = fr_in(w + 4, mont), gamma = fr_in(w + 8, mont), delta = fr_in(w + 12, mont), eta = fr_in(w + 16, mont), t = fr_in(w + 20, mont);
    const size_t nv = r.num_vars, n_inst = r.num_inputs, n_wit = nv - n_inst;
    if (cw > n_wit) return DGPU_E_BADARG;                                               // InsufficientWitnessesForCommitment (generator.rs:289-294)
    if (fr_is_zero(gamma) || fr_is_zero(delta)) return DGPU_E_BADARG;                   // UnexpectedIdentity
    const size_t n_abc = n_inst + cw, n_l = nv - n_abc;
    if (!o.gamma_abc || o.gamma_abc_cap < n_abc) return DGPU_E_BADARG;
    Domain d;
    int32_t rc;
    if ((rc = domain_for(r, t, d))) return rc;
    const size_t D = d.D, nh = D - 1;
    const FrH gi = gamma.inv(), di = delta.inv();
    CtxScope on_owner(href.h.ctx);
    // the two window tables (the generators' 8-bit windows): built and freed by this call
    struct Tab { uint64_t h = 0; ~Tab() { if (h) (void)dgpu_window_table_free(h); } } t1, t2;
    if ((rc = dgpu_window_table_g1(g1, &t1.h))) return rc;
    if ((rc = dgpu_window_table_g2(g2, &t2.h))) return rc;
    HandleRef r1(t1.h), r2(t2.h);
    if (!r1.ok || !r2.ok) return DGPU_E_BADARG;
    Keep keep;
    {
        SLOT_ACQUIRE(L, sl);
        HIPCHK(hipSetDevice(cur().device));
        hipStream_t s = sl.stream;
        size_t nnz[3];
        if ((rc = real_nnz(sl, r, nnz))) return rc;
        const size_t words_bytes = (2 * nv + n_abc + n_l + nh + 16) * 32 + 8 * 256;
        Block blk; blk.s = s;
        if (dev_malloc(&blk.p, im_bytes(r, D, nnz) + words_bytes) != hipSuccess) { (void)hipGetLastError(); blk.p = nullptr; return DGPU_E_OOM; }
        Carve cv{(uint8_t *)blk.p};
        ImOut im;
        if ((rc = instance_map_device(sl, r, t, d, nnz, cv, im))) return rc;
        uint32_t *a_w = cv.take<uint32_t>(nv * 32), *b_w = cv.take<uint32_t>(nv * 32), *abc_w = cv.take<uint32_t>(n_abc * 32 + 32), *l_w = cv.take<uint32_t>(n_l * 32 + 32);
        uint32_t *h_w = cv.take<uint32_t>(nh * 32 + 32), *small = cv.take<uint32_t>(16 * 32);
        // small: [alpha, beta, 1/gamma, 1/delta | Z(t)/delta | g1: alpha, beta, delta, eta/gamma, eta/delta, a0, b0 | g2: beta, delta, gamma, b0]
        uint64_t k[16][4] = {};
        alpha.to_canonical(k[0]); beta.to_canonical(k[1]); gi.to_canonical(k[2]); di.to_canonical(k[3]); (d.zt * di).to_canonical(k[4]);
        alpha.to_canonical(k[5]); beta.to_canonical(k[6]); delta.to_canonical(k[7]); (eta * gi).to_canonical(k[8]); (eta * di).to_canonical(k[9]);
        beta.to_canonical(k[12]); delta.to_canonical(k[13]); gamma.to_canonical(k[14]);
        HIPCHK(hipMemcpyAsync(small, k, sizeof k, hipMemcpyHostToDevice, s));
        setupk::launch_key_scalars(s, im.a, im.b, im.c, nv, n_abc, small, a_w, b_w, abc_w, l_w);
        if (nh) ntt::launch_fr_powers(s, im.consts + 16, small + 4 * 8, nh, im.pw);       // (Z(t) / delta) t^i, i < D - 1 (pw: free again)
        setupk::launch_soa_to_words(s, im.pw, nh, 0, h_w);
        HIPCHK(hipMemcpyAsync(small + 10 * 8, a_w, 32, hipMemcpyDeviceToDevice, s));     // a[0], b[0]: the query[0] the prover adds
        HIPCHK(hipMemcpyAsync(small + 11 * 8, b_w, 32, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(small + 15 * 8, b_w, 32, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipGetLastError());
        {
            StageTimer st(sl, "setup.fixed_base");
            const void *T1 = r1.h.p, *T2 = r2.h.p;
            if ((rc = table_mul_device<G2>(sl, T2, b_w, nv, &keep.p[2], o.xy[2], o.inf[2]))) return rc;     // generator.rs:337-339
            if ((rc = table_mul_device<G1>(sl, T1, a_w, nv, &keep.p[0], o.xy[0], o.inf[0]))) return rc;           // :357
            if ((rc = table_mul_device<G1>(sl, T1, b_w, nv, &keep.p[1], o.xy[1], o.inf[1]))) return rc;     // :363
            if ((rc = table_mul_device<G1>(sl, T1, h_w, nh, &keep.p[3], o.xy[3], o.inf[3]))) return rc;           // :369-376
            if ((rc = table_mul_device<G1>(sl, T1, l_w, n_l, &keep.p[4], o.xy[4], o.inf[4]))) return rc;          // :382
            std::vector<uint8_t> inf(std::max<size_t>(n_abc, 8));
            if ((rc = table_mul_device<G1>(sl, T1, abc_w, n_abc, nullptr, o.gamma_abc, inf.data()))) return rc;            // :406
            if ((rc = table_mul_device<G1>(sl, T1, small + 5 * 8, 7, nullptr, o.g1, inf.data()))) return rc;                     // :349-352,411,433
            if ((rc = table_mul_device<G2>(sl, T2, small + 12 * 8, 4, nullptr, o.g2, inf.data()))) return rc;                    // :351,353,405
        }
        if (hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); return DGPU_E_HIP; }
        if (gs.prof) prof_flush(sl);
    }
    // registered last: a failing call leaves no handle behind
    const size_t ns[5] = {nv, nv, nv, nh, n_l};
    const int kinds[5] = {1, 1, 2, 1, 1};
    for (int q = 0; q < 5; q++) { o.handles[q] = register_handle(keep.p[q], ns[q], kinds[q]); keep.p[q] = nullptr; }
    if (o.domain_size) *o.domain_size = D;
    (void)reserve_slots<G1>(2, std::max(nv, nh), 0, nullptr);        // as dgpu_window_table_mul_to_bases_* does: the prover's workspace exists before its first call
    (void)reserve_slots<G2>(2, nv, 0, nullptr);
    return DGPU_OK;
}

int32_t instance_map(uint64_t r1cs, const uint64_t *tw, int32_t montgomery, uint64_t *oa, uint64_t *ob, uint64_t *oc, uint64_t *ozt, size_t *oD) {
    if (!tw) return DGPU_E_BADARG;
    if (!cur().ready) return DGPU_E_NODEVICE;
    HandleRef href(r1cs);
    if (!href.ok || href.h.kind != 4) return DGPU_E_BADARG;
    const R1csView r = r1cs_view(href.h.p);
    const bool mont = montgomery != 0;
    const FrH t = fr_in(tw, mont);
    Domain d;
    int32_t rc;
    if ((rc = domain_for(r, t, d))) return rc;
    CtxScope on_owner(href.h.ctx);
    SLOT_ACQUIRE(L, sl);
    HIPCHK(hipSetDevice(cur().device));
    hipStream_t s = sl.stream;
    const size_t nv = r.num_vars;
    size_t nnz[3];
    if ((rc = real_nnz(sl, r, nnz))) return rc;
    Block blk; blk.s = s;
    if (dev_malloc(&blk.p, im_bytes(r, d.D, nnz) + 3 * (nv * 32 + 256)) != hipSuccess) { (void)hipGetLastError(); blk.p = nullptr; return DGPU_E_OOM; }
    Carve cv{(uint8_t *)blk.p};
    ImOut im;
    if ((rc = instance_map_device(sl, r, t, d, nnz, cv, im))) return rc;
    uint32_t *srcs[3] = {im.a, im.b, im.c};
    uint64_t *dsts[3] = {oa, ob, oc};
    for (int k = 0; k < 3; k++) {
        if (!dsts[k]) continue;
        uint32_t *wds = cv.take<uint32_t>(nv * 32);
        setupk::launch_soa_to_words(s, srcs[k], nv, mont, wds);
        if (nv && hipMemcpyAsync(dsts[k], wds, nv * 32, hipMemcpyDeviceToHost, s) != hipSuccess) { (void)hipGetLastError(); return DGPU_E_HIP; }
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); return DGPU_E_HIP; }
    if (gs.prof) prof_flush(sl);
    if (ozt) fr_out(d.zt, mont, ozt);
    if (oD) *oD = d.D;
    return DGPU_OK;
}

}  // namespace

extern "C" {
int32_t dgpu_qap_instance_map(uint64_t r1cs, const uint64_t t[4], int32_t montgomery, uint64_t *out_a, uint64_t *out_b, uint64_t *out_c, uint64_t out_zt[4], size_t *out_domain_size) {
    return abi_guard([&] { return instance_map(r1cs, t, montgomery, out_a, out_b, out_c, out_zt, out_domain_size); });
}
int32_t dgpu_legogroth16_setup(uint64_t r1cs, size_t commit_witness_count, const uint64_t waste[24], const uint64_t g1_xy[12], const uint64_t g2_xy[24],
                               int32_t montgomery, uint64_t out_handles[5], uint64_t *out_g1, uint64_t *out_g2, uint64_t *gamma_abc_g1, size_t gamma_abc_cap,
                               uint64_t **query_xy, uint8_t **query_inf, size_t *out_domain_size) {
    SetupOut o{out_handles, out_g1, out_g2, gamma_abc_g1, gamma_abc_cap, {}, {}, out_domain_size};
    for (int q = 0; q < 5; q++) { o.xy[q] = query_xy ? query_xy[q] : nullptr; o.inf[q] = query_inf ? query_inf[q] : nullptr; }
    return abi_guard([&] { return setup(r1cs, commit_witness_count, waste, g1_xy, g2_xy, montgomery, o); });
}
}  // extern "C"
