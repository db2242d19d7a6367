//! rust/dock_gpu/src/accumulator_proofs.rs — the VERIFIER of accumulator proofs in bulk (feature `vb-accumulator`, which brings the reference's `vb_accumulator`
//! crate in; the manager's side lives in accumulator_issue.rs and host.rs): the CDH proofs of vb_accumulator/src/proofs_cdh.rs against ONE accumulator value
//!
//!   `proof.verify(&V, &challenge, pk, params)`, n times (`MembershipProof`, proofs_cdh.rs:138-149)               -> `membership_verify_each`: the reference's first error per proof
//!   `proof.verify_partial(&resp_for_element, ..)`                                                                -> the same with `resp_for_element[i]` given
//!   the same with one verdict for all                                                                             -> `membership_verify_batch`
//!   `proof.verify(V, &challenge, pk, params, Q)`, n times (`NonMembershipProof`, proofs_cdh.rs:365-387, :481-523) -> `non_membership_verify_each`
//!   the same with one verdict for all                                                                             -> `non_membership_verify_batch`
//!
//! The KB universal accumulator's CDH proofs wrap the same `MembershipProof` (kb_universal_accumulator/proofs_cdh.rs): its two proof kinds go through the
//! membership calls.  `GpuAccumulatorVerifier` keeps the prepared coefficients of `pk` and `P~`: one preparation per key.
//! Every function answers `None` when the library declines (no device, a bad argument), so that the caller stays on the arkworks path it replaced.
//! NOT compiled in the build image (no Rust toolchain there); `tests/parity.rs` `accumulator_proofs_bulk_equal_the_reference` compares with the reference's own
//! `verify`.
use crate::ffi::*;
use crate::host::{raw_accumulator_membership_proofs_verify_batch, raw_accumulator_membership_proofs_verify_each, raw_accumulator_non_membership_proofs_verify_batch,
                  raw_accumulator_non_membership_proofs_verify_each};
use crate::{pack_g1, pack_g2, G2_PREPARED_WORDS};
use ark_bls12_381::{Bls12_381, Fr, G1Affine};
use ark_std::vec::Vec;
use schnorr_pok::error::SchnorrError;
use short_group_sig::error::ShortGroupSigError;
use vb_accumulator::error::VBAccumulatorError;
use vb_accumulator::proofs_cdh::{MembershipProof, NonMembershipProof};
use vb_accumulator::setup::{PublicKey, SetupParams};

/// the verifier's half of an accumulator key: `params.P` and the prepared coefficients of `pk = alpha P~` and of `P~`
pub struct GpuAccumulatorVerifier { p: G1Affine, pk_pc: Vec<u64>, ptilde_pc: Vec<u64> }
impl GpuAccumulatorVerifier {
    /// `None` for an identity `pk` or `P~`, or when the library declines
    pub fn new(params: &SetupParams<Bls12_381>, pk: &PublicKey<Bls12_381>) -> Option<Self> {
        let (q, qi) = pack_g2(&[pk.0, params.P_tilde]);
        let (mut co, mut inf) = (ark_std::vec![0u64; 2 * G2_PREPARED_WORDS], [0u8; 2]);
        if unsafe { dgpu_g2_prepare(q.as_ptr(), qi.as_ptr(), 2, co.as_mut_ptr(), inf.as_mut_ptr()) } != DGPU_OK || inf != [0u8; 2] { return None; }
        let ptilde_pc = co.split_off(G2_PREPARED_WORDS);
        Some(GpuAccumulatorVerifier { p: params.P, pk_pc: co, ptilde_pc })
    }
}

// the arrays of the C ABI for n membership proofs: (A', Abar, T) and (z1, z2); z2 from the full response, or `resp_for_element[i]` beside a partial one.
// `None` where the reference answers NeedEitherPartialOrCompleteSchnorrResponse (the wrong kind of response for the call, or none)
fn pack_membership(proofs: &[MembershipProof<Bls12_381>], resp_for_element: Option<&[Fr]>) -> Option<(Vec<u64>, Vec<Fr>)> {
    let (mut pts, mut resp) = (Vec::with_capacity(3 * proofs.len()), Vec::with_capacity(2 * proofs.len()));
    for (i, p) in proofs.iter().enumerate() {
        let (t, z1, z2) = match (resp_for_element, &p.0.sc, &p.0.sc_partial) {
            (None, Some(sc), _) => (sc.t, sc.response1, sc.response2),
            (Some(r), _, Some(sc)) => (sc.t, sc.response1, r[i]),
            _ => return None,
        };
        pts.extend_from_slice(&[p.0.A_prime, p.0.A_bar, t]);
        resp.extend_from_slice(&[z1, z2]);
    }
    Some((pack_g1(&pts).0, resp))                       // identity: zero words
}
fn membership_result(status: u8) -> Result<(), VBAccumulatorError> {
    // (all three checks of PoKOfSignatureG1::verify answer InvalidProof: weak_bb_sig_pok_cdh.rs:200-211, :283-285)
    if status == 0 { Ok(()) } else { Err(VBAccumulatorError::ShortGroupSigError(ShortGroupSigError::InvalidProof)) }
}

/// `proofs[i].verify(accumulator, &challenges[i], pk, params)` for every i (`verify_partial` with `resp_for_element[i]` where given).  The points are taken as
/// validated, as the reference takes them.
pub fn membership_verify_each(key: &GpuAccumulatorVerifier, accumulator: &G1Affine, proofs: &[MembershipProof<Bls12_381>], challenges: &[Fr], resp_for_element: Option<&[Fr]>)
                              -> Option<Vec<Result<(), VBAccumulatorError>>> {
    let n = proofs.len();
    if challenges.len() != n || resp_for_element.map_or(false, |r| r.len() != n) { return None; }
    let (pts, resp) = pack_membership(proofs, resp_for_element)?;
    let mut status = ark_std::vec![0u8; n];
    if raw_accumulator_membership_proofs_verify_each(accumulator, &key.pk_pc, &key.ptilde_pc, &pts, &resp, challenges, &mut status) != DGPU_OK { return None; }
    Some(status.into_iter().map(membership_result).collect())
}

/// all of them at once: one G1 equation and one pairing check under the weights `random^i`, `random` non-zero; no proofs at all verify
pub fn membership_verify_batch(key: &GpuAccumulatorVerifier, accumulator: &G1Affine, proofs: &[MembershipProof<Bls12_381>], challenges: &[Fr], resp_for_element: Option<&[Fr]>,
                               random: &Fr) -> Option<bool> {
    let n = proofs.len();
    if challenges.len() != n || resp_for_element.map_or(false, |r| r.len() != n) { return None; }
    let (pts, resp) = pack_membership(proofs, resp_for_element)?;
    let mut ok = 0i32;
    if raw_accumulator_membership_proofs_verify_batch(accumulator, &key.pk_pc, &key.ptilde_pc, &pts, &resp, challenges, random, &mut ok) != DGPU_OK { return None; }
    Some(ok != 0)
}

// (C', Cbar, J, T1, T2) and (s_r, s_y, s_d) of n non-membership proofs; s_y from sc_resp_1, or `resp_for_element[i]` where the proof is partial.  `None` where the
// reference answers MissingSchnorrResponseForElement or an error of pre_verify (a response count other than three, no response for r)
fn pack_non_membership(proofs: &[NonMembershipProof<Bls12_381>], resp_for_element: Option<&[Fr]>) -> Option<(Vec<u64>, Vec<Fr>)> {
    let (mut pts, mut resp) = (Vec::with_capacity(5 * proofs.len()), Vec::with_capacity(3 * proofs.len()));
    for (i, p) in proofs.iter().enumerate() {
        if p.sc_resp_1.total_responses != 3 { return None; }
        let s_r = *p.sc_resp_1.responses.get(&0)?;
        let s_y = match (p.sc_resp_1.responses.get(&1), resp_for_element) { (Some(z), _) => *z, (None, Some(r)) => r[i], (None, None) => return None };
        pts.extend_from_slice(&[p.C_prime, p.C_bar, p.J, p.t_1, p.sc_2.t]);
        resp.extend_from_slice(&[s_r, s_y, p.sc_2.response]);
    }
    Some((pack_g1(&pts).0, resp))
}
fn non_membership_result(status: u8) -> Result<(), VBAccumulatorError> {
    match status {
        0 => Ok(()),
        1 | 2 => Err(VBAccumulatorError::CannotBeZero),                               // proofs_cdh.rs:489-494
        3 => Err(VBAccumulatorError::IncorrectRandomizedWitness),                     // :495-497
        4 => Err(VBAccumulatorError::SchnorrError(SchnorrError::InvalidResponse)),    // :509-519, partial.rs:149-166
        _ => Err(VBAccumulatorError::IncorrectRandomizedWitness),                     // :375-385
    }
}

/// `proofs[i].verify(accumulator, &challenges[i], pk, params, q)` for every i (`verify_partial` with `resp_for_element[i]` where the proof lacks the element's
/// response)
pub fn non_membership_verify_each(key: &GpuAccumulatorVerifier, accumulator: &G1Affine, q: &G1Affine, proofs: &[NonMembershipProof<Bls12_381>], challenges: &[Fr],
                                  resp_for_element: Option<&[Fr]>) -> Option<Vec<Result<(), VBAccumulatorError>>> {
    let n = proofs.len();
    if challenges.len() != n || resp_for_element.map_or(false, |r| r.len() != n) { return None; }
    let (pts, resp) = pack_non_membership(proofs, resp_for_element)?;
    let mut status = ark_std::vec![0u8; n];
    if raw_accumulator_non_membership_proofs_verify_each(accumulator, &key.p, q, &key.pk_pc, &key.ptilde_pc, &pts, &resp, challenges, &mut status) != DGPU_OK { return None; }
    Some(status.into_iter().map(non_membership_result).collect())
}

/// all of them at once under the weights `random^(2i)` (the five-term check), `random^(2i+1)` (the check of J) and `random^i` (the pairing), `random` non-zero
pub fn non_membership_verify_batch(key: &GpuAccumulatorVerifier, accumulator: &G1Affine, q: &G1Affine, proofs: &[NonMembershipProof<Bls12_381>], challenges: &[Fr],
                                   resp_for_element: Option<&[Fr]>, random: &Fr) -> Option<bool> {
    let n = proofs.len();
    if challenges.len() != n || resp_for_element.map_or(false, |r| r.len() != n) { return None; }
    let (pts, resp) = pack_non_membership(proofs, resp_for_element)?;
    let mut ok = 0i32;
    if raw_accumulator_non_membership_proofs_verify_batch(accumulator, &key.p, q, &key.pk_pc, &key.ptilde_pc, &pts, &resp, challenges, random, &mut ok) != DGPU_OK { return None; }
    Some(ok != 0)
}
