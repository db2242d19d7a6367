// tests/native/msm_host_fold_driver.cpp — the host-side folds of the MSM driver (crypto_amd/csrc/msm_host_fold.hpp) as a program of their own, built with
// the host compiler from that header alone.  tests/test_msm_host_fold.py writes the cases, runs it (once more under AddressSanitizer + UBSan) and compares
// the results with the oracle.
//   msm_host_fold_driver g1|g2 IN OUT
// IN, u64 words: the number of cases, then per case  op, p0, p1, p2  and the operands; OUT: per case the return code and the 3 field elements of the result.
//   op 1 host_fold            p0 = W, p1 = c          W points (XYZZ), W flags
//   op 2 host_fold_shared     p0 = PW, p1 = lb        PW points A_j, PW flags, PW points S_j, PW flags
//   op 3 host_fold_marginals  p0 = nm, p1 = shift     1 + nm points, 1 + nm flags
//   op 4 host_fold_jacobian   p0 = k                  k Jacobian triples
//   op 5 host_lincomb         p0 = k, p1 = has flags  k affine points, k flags, k scalars of 4 words
// (a flag is one word in the file.)  Every operand array is copied into an allocation of exactly its size, so that a read past its end is the sanitizer's to see.
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../crypto_amd/csrc/msm_host_fold.hpp"

static std::vector<uint64_t> in;
static size_t pos = 0;
static std::vector<uint64_t> words(size_t n) {
    if (pos + n > in.size()) { fprintf(stderr, "msm_host_fold_driver: short input\n"); exit(2); }
    std::vector<uint64_t> v(in.begin() + pos, in.begin() + pos + n); pos += n; return v;
}
static std::vector<uint8_t> flags(size_t n) { std::vector<uint64_t> w = words(n); return std::vector<uint8_t>(w.begin(), w.end()); }

template <class HF> static int run(FILE *out) {
    const size_t F = sizeof(HF) / 8;
    const size_t ncase = words(1)[0];
    for (size_t i = 0; i < ncase; i++) {
        const std::vector<uint64_t> h = words(4);
        const size_t p0 = h[1]; const int p1 = (int)h[2];
        std::vector<uint64_t> res(3 * F, 0);
        int32_t rc = DGPU_OK;
        switch (h[0]) {
        case 1: { auto pts = words(p0 * 4 * F); auto inf = flags(p0); dock::host_fold<HF>(pts.data(), inf.data(), (int)p0, p1, res.data()); break; }
        case 2: { auto a = words(p0 * 4 * F); auto ai = flags(p0); auto s = words(p0 * 4 * F); auto si = flags(p0);
                  dock::host_fold_shared<HF>(a.data(), ai.data(), s.data(), si.data(), (int)p0, p1, res.data()); break; }
        case 3: { auto pts = words((p0 + 1) * 4 * F); auto inf = flags(p0 + 1); dock::host_fold_marginals<HF>(pts.data(), inf.data(), (int)p0, p1, res.data()); break; }
        case 4: { auto xyz = words(p0 * 3 * F); rc = dock::host_fold_jacobian<HF>(p0 ? xyz.data() : nullptr, p0, res.data()); break; }
        case 5: { auto pts = words(p0 * 2 * F); auto inf = flags(p0); auto sc = words(p0 * 4);
                  rc = dock::host_lincomb<HF>(p0 ? pts.data() : nullptr, p1 ? inf.data() : nullptr, p0 ? sc.data() : nullptr, p0, res.data()); break; }
        default: fprintf(stderr, "msm_host_fold_driver: unknown op\n"); return 2;
        }
        const uint64_t rcw = (uint64_t)(int64_t)rc;
        fwrite(&rcw, 8, 1, out); fwrite(res.data(), 8, res.size(), out);
    }
    return pos == in.size() ? 0 : 2;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *f = fopen(argv[2], "rb"); if (!f) return 2;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    in.resize((size_t)bytes / 8);
    if (fread(in.data(), 8, in.size(), f) != in.size()) return 2;
    fclose(f);
    FILE *out = fopen(argv[3], "wb"); if (!out) return 2;
    const int rc = !strcmp(argv[1], "g2") ? run<hostf::Fq2>(out) : run<hostf::Fq>(out);
    fclose(out);
    if (!rc) printf("msm_host_fold_driver: ok\n");
    return rc;
}
