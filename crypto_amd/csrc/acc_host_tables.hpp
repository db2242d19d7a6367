// crypto_amd/csrc/acc_host_tables.hpp — the host's share of the accumulator witness update (dock_accumulator.hip): the tables that depend on the secret key.
// Host-only and free of HIP, so that tests/native/acc_dev_host_shim.cpp compiles it as it is (tests/test_acc_device_code_on_host.py compares the tables
// with big integers).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "host_field.hpp"
#include "../../include/dock_gpu.h"

namespace acch {
using hostf::FrH;
using hostf::u128;

// 4 words -> field element in Montgomery form: canonical (any value below 2^256, reduced) or ark-ff Montgomery limbs
inline FrH fr_in(const uint64_t w[4], bool mont) {
    FrH a, r2, one{{1, 0, 0, 0}}; memcpy(a.l, w, 32); memcpy(r2.l, FrH::R2, 32);
    FrH x = a * r2;
    return mont ? x * one : x;
}
inline bool fr_is_zero(const FrH &x) { return (x.l[0] | x.l[1] | x.l[2] | x.l[3]) == 0; }
inline FrH fr_plus(const FrH &a, const FrH &b) {                 // both < r
    FrH s; uint64_t c = 0;
    for (int i = 0; i < 4; i++) { u128 t = (u128)a.l[i] + b.l[i] + c; s.l[i] = (uint64_t)t; c = (uint64_t)(t >> 64); }
    bool ge = c != 0;
    if (!ge) { ge = true; for (int i = 3; i >= 0; i--) { if (s.l[i] > FrH::MOD[i]) break; if (s.l[i] < FrH::MOD[i]) { ge = false; break; } } }
    if (ge) { uint64_t br = 0; for (int i = 0; i < 4; i++) { u128 d = (u128)s.l[i] - FrH::MOD[i] - br; s.l[i] = (uint64_t)d; br = (uint64_t)(d >> 64) & 1; } }
    return s;
}
inline void wipe(void *p, size_t bytes) { volatile uint8_t *q = (volatile uint8_t *)p; for (size_t i = 0; i < bytes; i++) q[i] = 0; }
// host words that depend on the secret key (the inverses 1 / (y + alpha), 1 / (x + e)): wiped when the call ends
struct SecretWords {
    std::vector<uint64_t> w;
    ~SecretWords() { if (!w.empty()) wipe(w.data(), w.size() * 8); }
};
// the host's tables as ark-ff Montgomery words, [a | F | r | G | Phi]; wiped when the call ends
struct Tables {
    std::vector<uint64_t> w;
    ~Tables() { if (!w.empty()) wipe(w.data(), w.size() * 8); }
};
// DGPU_E_BADARG for an addition or a removal equal to -alpha: F would hold a zero from there on, G would need its inverse (the reference computes garbage there)
inline int32_t build_tables(const uint64_t *additions, size_t na, const uint64_t *removals, size_t nr, const uint64_t alpha[4], bool mont, Tables &t) {
    t.w.assign((2 * na + 2 * nr + 1) * 4, 0);
    FrH *a = (FrH *)t.w.data(), *F = a + na, *r = F + na, *G = r + nr, *phi = G + nr;
    FrH al = fr_in(alpha, mont), acc = FrH::from_u64(1);
    int32_t rc = DGPU_OK;
    for (size_t s = 0; s < na && !rc; s++) {
        a[s] = fr_in(additions + 4 * s, mont);
        const FrH u = fr_plus(a[s], al);
        if (fr_is_zero(u)) rc = DGPU_E_BADARG;
        F[s] = acc; acc = acc * u;
    }
    *phi = acc;
    // G_s = 1 / prod_{i <= s} (r_i + alpha): the prefix products, ONE inversion, then back down (1 / Q_{s-1} = (r_s + alpha) / Q_s); r_s + alpha is parked in G_s meanwhile
    acc = FrH::from_u64(1);
    for (size_t s = 0; s < nr && !rc; s++) {
        r[s] = fr_in(removals + 4 * s, mont);
        G[s] = fr_plus(r[s], al);
        if (fr_is_zero(G[s])) rc = DGPU_E_BADARG;
        acc = acc * G[s];
    }
    if (!rc && nr) {
        FrH inv = acc.inv();
        for (size_t s = nr; s-- > 0;) { const FrH u = G[s]; G[s] = inv; inv = inv * u; }
    }
    wipe(&al, sizeof al); wipe(&acc, sizeof acc);
    return rc;
}
// the host's share of issuing witnesses (universal.rs:511-513, positive.rs:375-376): t_i = 1 / (y_i + alpha) for the entries [lo, hi), as ark-ff Montgomery
// words at t + 4 i, with ONE inversion (Montgomery's trick: t holds the prefix products in between).  DGPU_E_BADARG for a y_i equal to -alpha, which has no
// inverse (the reference's batch_inversion would leave a zero there and issue the identity).  zero != NULL (BBS+ signing, dock_bbs.hip: x + e_i = 0 is where
// SignatureG1::new draws e again, bbs_plus/src/signature.rs:178-181): such an entry is no error; zero[i] = 1 and t_i = 0 mark it, it stays out of the running
// product, and every other entry gets zero[i] = 0 and its inverse
inline int32_t issue_inverses(const uint64_t *ys, size_t lo, size_t hi, const uint64_t alpha[4], bool mont, uint64_t *t, uint8_t *zero = nullptr) {
    FrH al = fr_in(alpha, mont), acc = FrH::from_u64(1);
    int32_t rc = DGPU_OK;
    for (size_t i = lo; i < hi && !rc; i++) {
        const FrH u = fr_plus(fr_in(ys + 4 * i, mont), al);
        const bool z = fr_is_zero(u);
        if (zero) zero[i] = z ? 1 : 0;
        else if (z) rc = DGPU_E_BADARG;
        memcpy(t + 4 * i, acc.l, 32);
        if (!z) acc = acc * u;
    }
    if (!rc && hi > lo) {
        FrH inv = acc.inv();
        for (size_t i = hi; i-- > lo;) {
            if (zero && zero[i]) { memset(t + 4 * i, 0, 32); continue; }
            FrH u = fr_plus(fr_in(ys + 4 * i, mont), al), pre; memcpy(pre.l, t + 4 * i, 32);
            const FrH o = inv * pre; inv = inv * u;
            memcpy(t + 4 * i, o.l, 32);
            wipe(&u, sizeof u); wipe(&pre, sizeof pre);
        }
        wipe(&inv, sizeof inv);
    }
    wipe(&al, sizeof al); wipe(&acc, sizeof acc);
    return rc;
}
}  // namespace acch
