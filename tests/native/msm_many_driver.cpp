// tests/native/msm_many_driver.cpp — GPU parity driver for DeviceBases<G>::msm_many of the C++ host mirror (include/dock_gpu.hpp): m rows against the
// C ABI (dgpu_msm_*_handle_many), against m single calls (DeviceBases::msm_bigint) and against m MSMs of the CPU oracle (oracle/liboracle.so, test
// infrastructure).  Exit code 0 = all equal.
#include <cstdio>
#include <cstdlib>
#include "../../include/dock_gpu.hpp"

extern "C" {   // oracle/oracle.c
void orc_rand_scalars(uint64_t seed, size_t n, uint64_t *out);
void orc_g1_gen_seq(const uint64_t *k0, const uint64_t *d, size_t n, int threads, uint64_t *out);
void orc_g2_gen_seq(const uint64_t *k0, const uint64_t *d, size_t n, int threads, uint64_t *out);
void orc_g1_msm(const uint64_t *b, const uint8_t *inf, const uint64_t *s, size_t n, int threads, uint64_t *out);
void orc_g2_msm(const uint64_t *b, const uint8_t *inf, const uint64_t *s, size_t n, int threads, uint64_t *out);
int orc_g1_to_affine(const uint64_t *jac, uint64_t *out); int orc_g2_to_affine(const uint64_t *jac, uint64_t *out);
}
using namespace dock_gpu;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

template <class G> bool same_point(const typename G::Projective &got, const uint64_t *oracle_jac, int (*to_aff)(const uint64_t *, uint64_t *)) {
    uint64_t a[G::AW], b[G::AW], j[G::AW * 3 / 2];
    std::memcpy(j, &got.x, G::AW * 4); std::memcpy(j + G::AW / 2, &got.y, G::AW * 4); std::memcpy(j + G::AW, &got.z, G::AW * 4);
    int i1 = to_aff(j, a), i2 = to_aff(oracle_jac, b);
    return i1 == i2 && (i1 || std::memcmp(a, b, sizeof a) == 0);
}
template <class G> bool same_words(const typename G::Projective &a, const typename G::Projective &b) {
    return std::memcmp(&a.x, &b.x, G::AW * 4) == 0 && std::memcmp(&a.y, &b.y, G::AW * 4) == 0 && std::memcmp(&a.z, &b.z, G::AW * 4) == 0;
}

template <class G, class GEN, class MSM>
void run(size_t nb, size_t m, size_t n, size_t offset, GEN gen_seq, MSM orc_msm, int (*to_aff)(const uint64_t *, uint64_t *)) {
    constexpr size_t JW = G::AW * 3 / 2;
    std::vector<uint64_t> k0(4), d(4), sc(m * n * 4), b(nb * G::AW);
    orc_rand_scalars(11, 1, k0.data()); orc_rand_scalars(12, 1, d.data()); orc_rand_scalars(13 + m, m * n, sc.data());
    gen_seq(k0.data(), d.data(), nb, 8, b.data());
    auto P = affine_from_abi<G>(b, std::vector<uint8_t>(nb, 0));
    DeviceBases<G> q(P);
    std::vector<std::vector<BigInt256>> rows(m, std::vector<BigInt256>(n));
    for (size_t j = 0; j < m; j++) for (size_t i = 0; i < n; i++) std::memcpy(rows[j][i].data(), &sc[(j * n + i) * 4], 32);
    for (size_t i = 0; i < n; i++) rows[m / 2][i] = BigInt256{};                              // one identity row beside ordinary ones
    std::memset(&sc[(m / 2) * n * 4], 0, n * 32);
    auto got = q.msm_many(rows, offset);
    EXPECT(got.size() == m);
    std::vector<uint64_t> abi(m * JW); std::vector<uint8_t> inf(m, 7);
    EXPECT(G::msm_handle_many(q.handle(), offset, sc.data(), n, n, m, 0, abi.data(), inf.data()) == DGPU_OK);
    for (size_t j = 0; j < m && j < got.size(); j++) {
        EXPECT(same_words<G>(got[j], projective_from_abi<G>(&abi[j * JW])));
        EXPECT(same_words<G>(got[j], q.msm_bigint(rows[j], offset)));
        EXPECT(inf[j] == (got[j].is_zero() ? 1 : 0));
        EXPECT(got[j].is_zero() == (j == m / 2));
        uint64_t e[JW];
        orc_msm(b.data() + offset * G::AW, nullptr, &sc[j * n * 4], n, 8, e);
        EXPECT(same_point<G>(got[j], e, to_aff));
    }
    EXPECT(q.msm_many({}, 0).empty());                                                       // m = 0
}

int main() {
    init(0);
    run<G1>(300, 37, 24, 1, orc_g1_gen_seq, orc_g1_msm, orc_g1_to_affine);
    run<G1>(300, 5, 290, 3, orc_g1_gen_seq, orc_g1_msm, orc_g1_to_affine);
    run<G2>(100, 19, 7, 2, orc_g2_gen_seq, orc_g2_msm, orc_g2_to_affine);
    run<G2>(200, 3, 200, 0, orc_g2_gen_seq, orc_g2_msm, orc_g2_to_affine);
    if (fails) std::printf("msm_many_driver: %d FAILED\n", fails); else std::printf("msm_many_driver: all equal\n");
    return fails ? 1 : 0;
}
