//! rust/dock_gpu/src/smc_range_proof.rs — the VERIFIER of the reference's `smc_range_proof` crate in bulk (feature `smc-range-proof`, which brings that crate in):
//! BoundCheckSmc's two proofs over weak-BB signatures, for n proofs of ONE statement (min, max, base, params, commitment key)
//!
//!   `proof.verify(&commitment, &challenge, min, max, &comm_key, params)`, n times (`CLSRangeProof`, cls_range_proof/range_proof_cdh.rs:164-189)   -> `cls_verify_each`
//!   the same for `CCSArbitraryRangeProof` (ccs_range_proof/arbitrary_range_cdh.rs:210-250)                                                         -> `ccs_verify_each`
//!   `verify_given_randomized_pairing_checker` with one checker per proof (`random[i]` its scalar)                                                  -> the same with `Some(random)`
//!   one verdict for all under the weights `random^k`                                                                                              -> `cls_verify_batch`, `ccs_verify_batch`
//!
//! `GpuRangeVerifier` keeps g1, the commitment key and the prepared coefficients of the public key and of g2: one preparation per parameter set.  The
//! statement's constants follow the reference's rules (cls_range_proof/util.rs:15-93, ccs_range_proof/util.rs:6-78).  Every function answers `None` when the
//! library declines (no device, a bad argument), so that the caller stays on the arkworks path it replaced.  NOT compiled in the build image (no Rust toolchain
//! there); `tests/parity.rs` `smc_range_proofs_bulk_equal_the_reference` compares with the reference's own `verify`.
use crate::ffi::*;
use crate::{pack_g1, pack_g2, G2_PREPARED_WORDS};
use ark_bls12_381::{Bls12_381, Fr, G1Affine};
use ark_ff::Field;
use ark_std::vec::Vec;
use short_group_sig::error::ShortGroupSigError;
use short_group_sig::weak_bb_sig_pok_cdh::PoKOfSignatureG1;
use smc_range_proof::ccs_set_membership::setup::SetMembershipCheckParamsWithPairing;
use smc_range_proof::common::MemberCommitmentKey;
use smc_range_proof::error::SmcRangeProofError;
use smc_range_proof::prelude::{CCSArbitraryRangeProof, CLSRangeProof};

// include/dock_gpu_smc.h: served by libdock_gpu_smc.so — the product's objects plus these two calls — which a host that builds with this feature links INSTEAD
// of libdock_gpu.so (build.rs picks the library by the feature).  Declared here, by hand: ffi.rs is generated from include/dock_gpu.h alone.
extern "C" {
    fn dgpu_smc_range_proofs_verify_each_g1(g1: *const u64, ck_g: *const u64, ck_h: *const u64, pk_pc: *const u64, g2_pc: *const u64, sides: i32, l: usize, weights: *const u64,
                                            side_consts: *const u64, commitments: *const u64, digit_points: *const u64, digit_responses: *const u64, side_points: *const u64,
                                            side_responses: *const u64, challenge: *const u64, n: usize, montgomery: i32, random: *const u64, status: *mut u8, detail: *mut i32) -> i32;
    fn dgpu_smc_range_proofs_verify_batch_g1(g1: *const u64, ck_g: *const u64, ck_h: *const u64, pk_pc: *const u64, g2_pc: *const u64, sides: i32, l: usize, weights: *const u64,
                                             side_consts: *const u64, commitments: *const u64, digit_points: *const u64, digit_responses: *const u64, side_points: *const u64,
                                             side_responses: *const u64, challenge: *const u64, n: usize, montgomery: i32, random: *const u64, ok: *mut i32) -> i32;
}

/// the verifier's half of the parameters: g1, (g, h), the prepared coefficients of `bb_pk` and g2, and the set size `validate_base` compares with
pub struct GpuRangeVerifier { pts: Vec<u64>, pk_pc: Vec<u64>, g2_pc: Vec<u64>, max_base: u16 }
impl GpuRangeVerifier {
    /// `None` for an identity public key or g2, or when the library declines
    pub fn new(params: &SetMembershipCheckParamsWithPairing<Bls12_381>, comm_key: &MemberCommitmentKey<G1Affine>) -> Option<Self> {
        let (q, qi) = pack_g2(&[params.bb_pk.0, params.bb_sig_params.g2]);
        let (mut co, mut inf) = (ark_std::vec![0u64; 2 * G2_PREPARED_WORDS], [0u8; 2]);
        if unsafe { dgpu_g2_prepare(q.as_ptr(), qi.as_ptr(), 2, co.as_mut_ptr(), inf.as_mut_ptr()) } != DGPU_OK || inf != [0u8; 2] { return None; }
        let g2_pc = co.split_off(G2_PREPARED_WORDS);
        Some(GpuRangeVerifier { pts: pack_g1(&[params.bb_sig_params.g1, comm_key.g, comm_key.h]).0, pk_pc: co, g2_pc, max_base: params.get_max_base_for_range_proof() })
    }
}

/// (sides, l, weights, per side (a, b, e)) of a statement:  a c C + (b c + sum_j w_j z2_j) g + e zr h = D
pub struct Statement { sides: usize, l: usize, weights: Vec<Fr>, consts: Vec<Fr> }
fn check_bounds(key: &GpuRangeVerifier, min: u64, max: u64, base: u16) -> Result<(), SmcRangeProofError> {
    if key.max_base < base { return Err(SmcRangeProofError::UnsupportedBase(base, key.max_base)); }
    if min >= max { return Err(SmcRangeProofError::IncorrectBounds(ark_std::format!("min={} should be < max={}", min, max))); }
    Ok(())
}
/// `CLSRangeProof::verify`'s statement: check_commitment works on (min, max - 1)
pub fn cls_statement(key: &GpuRangeVerifier, min: u64, max: u64, base: u16) -> Result<Statement, SmcRangeProofError> {
    check_bounds(key, min, max, base)?;
    let (b1, mut range, mut rm) = ((base - 1) as u128, (max - 1 - min) as u128, 1u128);
    if range % b1 != 0 { range *= b1; rm = b1; }
    let bb = base as u128;
    let mut l = 0u32;
    while bb.checked_pow(l).map_or(false, |v| v < range + 1) { l += 1; }
    let g: Vec<u128> = if base == 2 { (0..l).map(|i| (range + (1 << i)) >> (i + 1)).collect() } else {
        let mut h = Vec::new();
        let mut v = range;
        while v != 0 { h.push(v % bb); v /= bb; }
        h.resize(l as usize, 0);
        (0..l as usize).map(|i| range / bb.pow(i as u32 + 1) + (1 + h[i] + h[..i].iter().sum::<u128>() % b1) / bb).collect()
    };
    Ok(Statement { sides: 1, l: l as usize, weights: g.into_iter().map(Fr::from).collect(), consts: ark_std::vec![-Fr::from(rm), Fr::from(min as u128 * rm), Fr::from(rm)] })
}
/// `CCSArbitraryRangeProof::verify`'s statement; base^l as an integer (the reference's u64 power overflows from base^l = 2^64 on)
pub fn ccs_statement(key: &GpuRangeVerifier, min: u64, max: u64, base: u16) -> Result<Statement, SmcRangeProofError> {
    check_bounds(key, min, max, base)?;
    let (bb, diff) = (base as u128, (max - min) as u128);
    let mut l = 0u32;
    while bb.pow(l) <= diff { l += 1; }
    let one = Fr::from(1u64);
    let x = Fr::from(bb.pow(l)) - Fr::from(max);
    Ok(Statement { sides: 2, l: l as usize, weights: (0..l as u64).map(|j| Fr::from(base).pow([j])).collect(), consts: ark_std::vec![-one, Fr::from(min), one, -one, -x, one] })
}

// the arrays of the C ABI for the digits of one side: (A', Abar, T) and (z1, z2).  `None` for a proof without the full Schnorr response
fn push_digits(sigs: &[PoKOfSignatureG1<Bls12_381>], pts: &mut Vec<G1Affine>, resp: &mut Vec<Fr>) -> Option<()> {
    for p in sigs {
        let sc = p.sc.as_ref()?;
        pts.extend_from_slice(&[p.A_prime, p.A_bar, sc.t]);
        resp.extend_from_slice(&[sc.response1, sc.response2]);
    }
    Some(())
}
struct Packed { commitments: Vec<u64>, digit_points: Vec<u64>, digit_resp: Vec<Fr>, side_points: Vec<u64>, side_resp: Vec<Fr> }
fn result_of(status: u8) -> Result<(), SmcRangeProofError> {
    match status {
        0 => Ok(()),
        1 => Err(SmcRangeProofError::InvalidRangeProof),
        _ => Err(SmcRangeProofError::ShortGroupSig(ShortGroupSigError::InvalidProof)),      // (2: a digit; 3: the merged pairing check, which the reference's checker reports at its end)
    }
}
fn each(key: &GpuRangeVerifier, st: &Statement, p: &Packed, challenges: &[Fr], random: Option<&[Fr]>) -> Option<Vec<Result<(), SmcRangeProofError>>> {
    let n = challenges.len();
    if random.map_or(false, |r| r.len() != n) { return None; }
    let (mut status, mut detail) = (ark_std::vec![0u8; n], ark_std::vec![0i32; n]);
    let rc = unsafe {
        dgpu_smc_range_proofs_verify_each_g1(key.pts.as_ptr(), key.pts[12..].as_ptr(), key.pts[24..].as_ptr(), key.pk_pc.as_ptr(), key.g2_pc.as_ptr(), st.sides as i32, st.l,
                                             st.weights.as_ptr() as *const u64, st.consts.as_ptr() as *const u64, p.commitments.as_ptr(), p.digit_points.as_ptr(),
                                             p.digit_resp.as_ptr() as *const u64, p.side_points.as_ptr(), p.side_resp.as_ptr() as *const u64, challenges.as_ptr() as *const u64, n, 1,
                                             random.map_or(core::ptr::null(), |r| r.as_ptr() as *const u64), status.as_mut_ptr(), detail.as_mut_ptr())
    };
    if rc != DGPU_OK { return None; }
    Some(status.into_iter().map(result_of).collect())
}
fn batch(key: &GpuRangeVerifier, st: &Statement, p: &Packed, challenges: &[Fr], random: &Fr) -> Option<bool> {
    let mut ok = 0i32;
    let rc = unsafe {
        dgpu_smc_range_proofs_verify_batch_g1(key.pts.as_ptr(), key.pts[12..].as_ptr(), key.pts[24..].as_ptr(), key.pk_pc.as_ptr(), key.g2_pc.as_ptr(), st.sides as i32, st.l,
                                              st.weights.as_ptr() as *const u64, st.consts.as_ptr() as *const u64, p.commitments.as_ptr(), p.digit_points.as_ptr(),
                                              p.digit_resp.as_ptr() as *const u64, p.side_points.as_ptr(), p.side_resp.as_ptr() as *const u64, challenges.as_ptr() as *const u64,
                                              challenges.len(), 1, random as *const Fr as *const u64, &mut ok)
    };
    if rc != DGPU_OK { None } else { Some(ok != 0) }
}
fn pack_cls(st: &Statement, commitments: &[G1Affine], proofs: &[CLSRangeProof<Bls12_381>]) -> Option<Packed> {
    let (mut dp, mut dr, mut sp, mut sr) = (Vec::new(), Vec::new(), Vec::new(), Vec::new());
    for p in proofs {
        if p.pok_sigs.len() != st.l { return None; }
        push_digits(&p.pok_sigs, &mut dp, &mut dr)?;
        sp.push(p.D); sr.push(p.resp_r);
    }
    Some(Packed { commitments: pack_g1(commitments).0, digit_points: pack_g1(&dp).0, digit_resp: dr, side_points: pack_g1(&sp).0, side_resp: sr })
}
// `Err(ProofShorterThanExpected)` where a side does not hold l digits, as verify_except_pairings answers (arbitrary_range_cdh.rs:327-337)
fn pack_ccs(st: &Statement, commitments: &[G1Affine], proofs: &[CCSArbitraryRangeProof<Bls12_381>]) -> Result<Option<Packed>, SmcRangeProofError> {
    let (mut dp, mut dr, mut sp, mut sr) = (Vec::new(), Vec::new(), Vec::new(), Vec::new());
    for p in proofs {
        if p.pok_sigs_min.len() != st.l || p.pok_sigs_max.len() != st.l { return Err(SmcRangeProofError::ProofShorterThanExpected); }
        if push_digits(&p.pok_sigs_min, &mut dp, &mut dr).is_none() || push_digits(&p.pok_sigs_max, &mut dp, &mut dr).is_none() { return Ok(None); }
        sp.extend_from_slice(&[p.D_min, p.D_max]); sr.extend_from_slice(&[p.resp_r_min, p.resp_r_max]);
    }
    Ok(Some(Packed { commitments: pack_g1(commitments).0, digit_points: pack_g1(&dp).0, digit_resp: dr, side_points: pack_g1(&sp).0, side_resp: sr }))
}

/// `proofs[i].verify(&commitments[i], &challenges[i], min, max, comm_key, params)` for every i; with `random`, `verify_given_randomized_pairing_checker` and
/// the checker's verdict, one checker per proof.  The points are taken as validated, as the reference takes them.
pub fn cls_verify_each(key: &GpuRangeVerifier, st: &Statement, commitments: &[G1Affine], proofs: &[CLSRangeProof<Bls12_381>], challenges: &[Fr], random: Option<&[Fr]>)
                       -> Option<Vec<Result<(), SmcRangeProofError>>> {
    if st.sides != 1 || commitments.len() != proofs.len() || challenges.len() != proofs.len() { return None; }
    each(key, st, &pack_cls(st, commitments, proofs)?, challenges, random)
}
/// all of them at once: one G1 equation and one pairing check, `random` non-zero; no proofs at all verify
pub fn cls_verify_batch(key: &GpuRangeVerifier, st: &Statement, commitments: &[G1Affine], proofs: &[CLSRangeProof<Bls12_381>], challenges: &[Fr], random: &Fr) -> Option<bool> {
    if st.sides != 1 || commitments.len() != proofs.len() || challenges.len() != proofs.len() { return None; }
    batch(key, st, &pack_cls(st, commitments, proofs)?, challenges, random)
}
pub fn ccs_verify_each(key: &GpuRangeVerifier, st: &Statement, commitments: &[G1Affine], proofs: &[CCSArbitraryRangeProof<Bls12_381>], challenges: &[Fr], random: Option<&[Fr]>)
                       -> Result<Option<Vec<Result<(), SmcRangeProofError>>>, SmcRangeProofError> {
    if st.sides != 2 || commitments.len() != proofs.len() || challenges.len() != proofs.len() { return Ok(None); }
    Ok(pack_ccs(st, commitments, proofs)?.and_then(|p| each(key, st, &p, challenges, random)))
}
pub fn ccs_verify_batch(key: &GpuRangeVerifier, st: &Statement, commitments: &[G1Affine], proofs: &[CCSArbitraryRangeProof<Bls12_381>], challenges: &[Fr], random: &Fr)
                        -> Result<Option<bool>, SmcRangeProofError> {
    if st.sides != 2 || commitments.len() != proofs.len() || challenges.len() != proofs.len() { return Ok(None); }
    Ok(pack_ccs(st, commitments, proofs)?.and_then(|p| batch(key, st, &p, challenges, random)))
}
