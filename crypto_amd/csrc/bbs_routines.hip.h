// crypto_amd/csrc/bbs_routines.hip.h — the BBS row, shared by the BBS+ scalar kernels (bbs_kernels.hip.h: signatures; bbs_pok_kernels.hip.h: proofs of knowledge),
// the 2023 scheme and PS: plain FRD functions over load / store functors, so the same text runs on the host under -DFP29_CHECK, where every product asserts its
// operand contract (tests/native/bbs_dev_host_shim.cpp, bbs_pok_dev_host_shim.cpp).  The column sums of the batch calls, the loads and stores of 8-word scalars
// and the operand classes ("product", "lazy sum") are col_sums.hip.h's.
#pragma once
#include "col_sums.hip.h"

namespace bbsk {
using namespace fr29;      // (col_sums.hip.h makes colk's names visible here)

// entry k of row i before its multiplier, with `fixed` columns in front of the messages: one, [s_i,] m_i(k-fixed).  fixed = 2: BBS+ (1, s_i, m_i ..);
// fixed = 1: the 2023 scheme (1, m_i ..), where s is never called.  s(i, Fr &) / m(i, j, Fr &) load products.
template <class S, class M> FRD void row_value_fixed(Fr &v, size_t i, size_t k, size_t fixed, S s, M m) {
    if (k == 0) fr_one(v); else if (k < fixed) s(i, v); else m(i, k - fixed, v);
}
// the BBS+ row: one, s_i, m_i(k-2)
template <class S, class M> FRD void row_value(Fr &v, size_t i, size_t k, S s, M m) { row_value_fixed(v, i, k, 2, s, m); }
// o = mult v.  v, mult: products (mult: t_i, or one)
FRD void row_entry(Fr &o, const Fr &v, const Fr &mult) { fr_mul(o, v, mult); }      // 2 r * 2 r

}  // namespace bbsk
