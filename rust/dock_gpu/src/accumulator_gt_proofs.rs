//! rust/dock_gpu/src/accumulator_gt_proofs.rs — the VERIFIER of the accumulator proofs with a GT commitment in bulk (feature `vb-accumulator`, which brings the
//! reference's `vb_accumulator` crate in): the proofs of vb_accumulator/src/proofs.rs — what `proof_system`'s statements VBAccumulatorMembership,
//! VBAccumulatorNonMembership and, through kb_universal_accumulator/proofs.rs, KBUniversalAccumulatorMembership / KBUniversalAccumulatorNonMembership carry —
//! against ONE accumulator value
//!
//!   `proof.verify(&V, &challenge, pk, params, prk)`, n times (`MembershipProof`, proofs.rs:1269-1290)      -> `membership_verify_each`: the reference's first error per proof
//!   `proof.verify_partial(&resp_for_element, ..)`                                                          -> the same with `resp_for_element[i]` given
//!   the same with one verdict for all                                                                       -> `membership_verify_batch`
//!   `proof.verify(&V, &challenge, pk, params, prk)`, n times (`NonMembershipProof`, proofs.rs:1393-1420)   -> `non_membership_verify_each`
//!   the same with one verdict for all                                                                       -> `non_membership_verify_batch`
//!
//! The KB universal accumulator's proofs wrap the same `MembershipProof`: its two proof kinds go through the membership calls.  `GpuAccumulatorGtVerifier`
//! keeps the prepared coefficients of `pk` and `P~`: one preparation per key.  Every function answers `None` when the library declines (no device, a bad
//! argument) or when the reference would answer MissingSchnorrResponseForElement, so that the caller stays on the arkworks path it replaced.
//! The four calls are served by libdock_gpu_acc_gt.so (include/dock_gpu_acc_gt.h), which exports everything libdock_gpu.so does: build.rs links it INSTEAD of the
//! product when `vb-accumulator` is the only feature that picks a library; beside `saver`, `smc-range-proof` or `bulletproofs-plus-plus` (each of which links
//! its own library) this module is left out (lib.rs).
//! NOT compiled in the build image (no Rust toolchain there); `tests/parity.rs` `accumulator_gt_proofs_bulk_equal_the_reference` compares with the reference's
//! own `verify`.
use crate::ffi::*;
use crate::{fq12_to_words, pack_g1, pack_g2, G2_PREPARED_WORDS};
use ark_bls12_381::{Bls12_381, Fr, G1Affine};
use ark_std::vec::Vec;
use vb_accumulator::error::VBAccumulatorError;
use vb_accumulator::proofs::{MembershipProof, NonMembershipProof, RandomizedWitness, SchnorrCommit, SchnorrResponse};
use vb_accumulator::setup::{NonMembershipProvingKey, ProvingKey, PublicKey, SetupParams};

// include/dock_gpu_acc_gt.h, declared here by hand: ffi.rs is generated from include/dock_gpu.h alone.
extern "C" {
    fn dgpu_accumulator_gt_membership_proofs_verify_each_g1(accumulator_xy: *const u64, prk_xy: *const u64, pk_pc: *const u64, ptilde_pc: *const u64, points: *const u64,
                                                            r_e: *const u64, responses: *const u64, challenge: *const u64, n: usize, montgomery: i32, status: *mut u8) -> i32;
    fn dgpu_accumulator_gt_membership_proofs_verify_batch_g1(accumulator_xy: *const u64, prk_xy: *const u64, pk_pc: *const u64, ptilde_pc: *const u64, points: *const u64,
                                                             r_e: *const u64, responses: *const u64, challenge: *const u64, n: usize, montgomery: i32, random: *const u64,
                                                             ok: *mut i32) -> i32;
    fn dgpu_accumulator_gt_non_membership_proofs_verify_each_g1(accumulator_xy: *const u64, p_xy: *const u64, prk_xy: *const u64, pk_pc: *const u64, ptilde_pc: *const u64,
                                                                points: *const u64, r_e: *const u64, responses: *const u64, challenge: *const u64, n: usize, montgomery: i32,
                                                                status: *mut u8) -> i32;
    fn dgpu_accumulator_gt_non_membership_proofs_verify_batch_g1(accumulator_xy: *const u64, p_xy: *const u64, prk_xy: *const u64, pk_pc: *const u64, ptilde_pc: *const u64,
                                                                 points: *const u64, r_e: *const u64, responses: *const u64, challenge: *const u64, n: usize, montgomery: i32,
                                                                 random: *const u64, ok: *mut i32) -> i32;
}

/// the verifier's half of an accumulator key: `params.P` and the prepared coefficients of `pk = alpha P~` and of `P~`
pub struct GpuAccumulatorGtVerifier { p: Vec<u64>, pk_pc: Vec<u64>, ptilde_pc: Vec<u64> }
impl GpuAccumulatorGtVerifier {
    /// `None` for an identity `pk` or `P~`, or when the library declines
    pub fn new(params: &SetupParams<Bls12_381>, pk: &PublicKey<Bls12_381>) -> Option<Self> {
        let (q, qi) = pack_g2(&[pk.0, params.P_tilde]);
        let (mut co, mut inf) = (ark_std::vec![0u64; 2 * G2_PREPARED_WORDS], [0u8; 2]);
        if unsafe { dgpu_g2_prepare(q.as_ptr(), qi.as_ptr(), 2, co.as_mut_ptr(), inf.as_mut_ptr()) } != DGPU_OK || inf != [0u8; 2] { return None; }
        let ptilde_pc = co.split_off(G2_PREPARED_WORDS);
        Some(GpuAccumulatorGtVerifier { p: pack_g1(&[params.P]).0, pk_pc: co, ptilde_pc })
    }
}

// Fr is four Montgomery limbs in memory: the calls take them as they stand (montgomery = 1)
fn fr_ptr(v: &[Fr]) -> *const u64 { v.as_ptr() as *const u64 }

// what the two kinds share of a proof: (E_C, T_sigma, T_rho, R_sigma, R_rho, R_delta_sigma, R_delta_rho), R_E, (s_sigma, s_rho, s_delta_sigma, s_delta_rho, s_y);
// s_y from the response, or `resp_for_element` beside a partial one.  `None`: MissingSchnorrResponseForElement (proofs.rs:901-907)
fn push_common(rw: &RandomizedWitness<G1Affine>, sc: &SchnorrCommit<Bls12_381>, sr: &SchnorrResponse<Fr>, resp_for_element: Option<Fr>, pts: &mut Vec<G1Affine>,
               r_e: &mut Vec<u64>, resp: &mut Vec<Fr>) -> Option<()> {
    let s_y = match (resp_for_element, sr.s_y) { (Some(r), _) => r, (None, Some(s)) => s, (None, None) => return None };      // (the reference prefers resp_for_element too)
    pts.extend_from_slice(&[rw.E_C, rw.T_sigma, rw.T_rho, sc.R_sigma, sc.R_rho, sc.R_delta_sigma, sc.R_delta_rho]);
    r_e.extend_from_slice(&fq12_to_words(&sc.R_E.0));
    resp.extend_from_slice(&[sr.s_sigma, sr.s_rho, sr.s_delta_sigma, sr.s_delta_rho, s_y]);
    Some(())
}
struct Packed { pts: Vec<u64>, r_e: Vec<u64>, resp: Vec<Fr> }
fn pack_membership(proofs: &[MembershipProof<Bls12_381>], resp_for_element: Option<&[Fr]>) -> Option<Packed> {
    let n = proofs.len();
    let (mut pts, mut r_e, mut resp) = (Vec::with_capacity(7 * n), Vec::with_capacity(72 * n), Vec::with_capacity(5 * n));
    for (i, p) in proofs.iter().enumerate() {
        push_common(&p.randomized_witness.0, &p.schnorr_commit.0, &p.schnorr_response.0, resp_for_element.map(|r| r[i]), &mut pts, &mut r_e, &mut resp)?;
    }
    Some(Packed { pts: pack_g1(&pts).0, r_e, resp })                    // identity: zero words
}
fn pack_non_membership(proofs: &[NonMembershipProof<Bls12_381>], resp_for_element: Option<&[Fr]>) -> Option<Packed> {
    let n = proofs.len();
    let (mut pts, mut r_e, mut resp) = (Vec::with_capacity(11 * n), Vec::with_capacity(72 * n), Vec::with_capacity(8 * n));
    for (i, p) in proofs.iter().enumerate() {
        push_common(&p.randomized_witness.C, &p.schnorr_commit.C, &p.schnorr_response.C, resp_for_element.map(|r| r[i]), &mut pts, &mut r_e, &mut resp)?;
        pts.extend_from_slice(&[p.randomized_witness.E_d, p.randomized_witness.E_d_inv, p.schnorr_commit.R_A, p.schnorr_commit.R_B]);
        resp.extend_from_slice(&[p.schnorr_response.s_u, p.schnorr_response.s_v, p.schnorr_response.s_w]);
    }
    Some(Packed { pts: pack_g1(&pts).0, r_e, resp })
}
// the order of the reference's errors (proofs.rs:1533-1549, :911-938, :717-721): `first` is the status of SigmaResponseInvalid, 1 or 3
fn result_of(status: u8, first: u8) -> Result<(), VBAccumulatorError> {
    if status == 0 { return Ok(()); }
    Err(match (status, status.wrapping_sub(first)) {
        (1, _) if first == 3 => VBAccumulatorError::E_d_ResponseInvalid,
        (2, _) if first == 3 => VBAccumulatorError::E_d_inv_ResponseInvalid,
        (_, 0) => VBAccumulatorError::SigmaResponseInvalid,
        (_, 1) => VBAccumulatorError::RhoResponseInvalid,
        (_, 2) => VBAccumulatorError::DeltaSigmaResponseInvalid,
        (_, 3) => VBAccumulatorError::DeltaRhoResponseInvalid,
        _ => VBAccumulatorError::PairingResponseInvalid,
    })
}
fn prk_words(prk: &ProvingKey<G1Affine>, k: Option<&G1Affine>) -> Vec<u64> {
    let mut v = ark_std::vec![prk.X, prk.Y, prk.Z];
    if let Some(k) = k { v.push(*k); }
    pack_g1(&v).0
}
fn lengths_ok(n: usize, challenges: &[Fr], resp_for_element: Option<&[Fr]>) -> bool { challenges.len() == n && resp_for_element.map_or(true, |r| r.len() == n) }

/// `proofs[i].verify(accumulator, &challenges[i], pk, params, prk)` for every i (`verify_partial` with `resp_for_element[i]` where given).  The points and the
/// GT elements are taken as validated, as the reference takes them after deserialising.
pub fn membership_verify_each(key: &GpuAccumulatorGtVerifier, accumulator: &G1Affine, prk: &ProvingKey<G1Affine>, proofs: &[MembershipProof<Bls12_381>], challenges: &[Fr],
                              resp_for_element: Option<&[Fr]>) -> Option<Vec<Result<(), VBAccumulatorError>>> {
    let n = proofs.len();
    if !lengths_ok(n, challenges, resp_for_element) { return None; }
    let (a, k, v) = (pack_membership(proofs, resp_for_element)?, prk_words(prk, None), pack_g1(&[*accumulator]).0);
    let mut status = ark_std::vec![0u8; n];
    let rc = unsafe { dgpu_accumulator_gt_membership_proofs_verify_each_g1(v.as_ptr(), k.as_ptr(), key.pk_pc.as_ptr(), key.ptilde_pc.as_ptr(), a.pts.as_ptr(), a.r_e.as_ptr(),
                                                                           fr_ptr(&a.resp), fr_ptr(challenges), n, 1, status.as_mut_ptr()) };
    if rc != DGPU_OK { return None; }
    Some(status.into_iter().map(|s| result_of(s, 1)).collect())
}

/// all of them at once: one G1 equation over every Schnorr check (check j of proof i weighs `random^(4 i + j)`) and one pairing check against the product of
/// the `R_E_i^(random^i)`; `random` non-zero; no proofs at all verify
pub fn membership_verify_batch(key: &GpuAccumulatorGtVerifier, accumulator: &G1Affine, prk: &ProvingKey<G1Affine>, proofs: &[MembershipProof<Bls12_381>], challenges: &[Fr],
                               resp_for_element: Option<&[Fr]>, random: &Fr) -> Option<bool> {
    let n = proofs.len();
    if !lengths_ok(n, challenges, resp_for_element) { return None; }
    let (a, k, v) = (pack_membership(proofs, resp_for_element)?, prk_words(prk, None), pack_g1(&[*accumulator]).0);
    let mut ok = 0i32;
    let rc = unsafe { dgpu_accumulator_gt_membership_proofs_verify_batch_g1(v.as_ptr(), k.as_ptr(), key.pk_pc.as_ptr(), key.ptilde_pc.as_ptr(), a.pts.as_ptr(), a.r_e.as_ptr(),
                                                                            fr_ptr(&a.resp), fr_ptr(challenges), n, 1, fr_ptr(core::slice::from_ref(random)), &mut ok) };
    if rc != DGPU_OK { return None; }
    Some(ok != 0)
}

/// `proofs[i].verify(accumulator, &challenges[i], pk, params, prk)` for every i (`verify_partial` with `resp_for_element[i]` where the proof lacks `s_y`)
pub fn non_membership_verify_each(key: &GpuAccumulatorGtVerifier, accumulator: &G1Affine, prk: &NonMembershipProvingKey<G1Affine>, proofs: &[NonMembershipProof<Bls12_381>],
                                  challenges: &[Fr], resp_for_element: Option<&[Fr]>) -> Option<Vec<Result<(), VBAccumulatorError>>> {
    let n = proofs.len();
    if !lengths_ok(n, challenges, resp_for_element) { return None; }
    let (a, k, v) = (pack_non_membership(proofs, resp_for_element)?, prk_words(&prk.XYZ, Some(&prk.K)), pack_g1(&[*accumulator]).0);
    let mut status = ark_std::vec![0u8; n];
    let rc = unsafe { dgpu_accumulator_gt_non_membership_proofs_verify_each_g1(v.as_ptr(), key.p.as_ptr(), k.as_ptr(), key.pk_pc.as_ptr(), key.ptilde_pc.as_ptr(), a.pts.as_ptr(),
                                                                               a.r_e.as_ptr(), fr_ptr(&a.resp), fr_ptr(challenges), n, 1, status.as_mut_ptr()) };
    if rc != DGPU_OK { return None; }
    Some(status.into_iter().map(|s| result_of(s, 3)).collect())
}

/// all of them at once under the weights `random^(6 i + j)` on Schnorr check j of proof i and `random^i` on its pairing and its `R_E`; `random` non-zero
pub fn non_membership_verify_batch(key: &GpuAccumulatorGtVerifier, accumulator: &G1Affine, prk: &NonMembershipProvingKey<G1Affine>, proofs: &[NonMembershipProof<Bls12_381>],
                                   challenges: &[Fr], resp_for_element: Option<&[Fr]>, random: &Fr) -> Option<bool> {
    let n = proofs.len();
    if !lengths_ok(n, challenges, resp_for_element) { return None; }
    let (a, k, v) = (pack_non_membership(proofs, resp_for_element)?, prk_words(&prk.XYZ, Some(&prk.K)), pack_g1(&[*accumulator]).0);
    let mut ok = 0i32;
    let rc = unsafe { dgpu_accumulator_gt_non_membership_proofs_verify_batch_g1(v.as_ptr(), key.p.as_ptr(), k.as_ptr(), key.pk_pc.as_ptr(), key.ptilde_pc.as_ptr(), a.pts.as_ptr(),
                                                                                a.r_e.as_ptr(), fr_ptr(&a.resp), fr_ptr(challenges), n, 1,
                                                                                fr_ptr(core::slice::from_ref(random)), &mut ok) };
    if rc != DGPU_OK { return None; }
    Some(ok != 0)
}
