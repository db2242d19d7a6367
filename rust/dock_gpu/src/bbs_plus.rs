//! rust/dock_gpu/src/bbs_plus.rs — the plain G1 BBS+ signature in bulk (feature `bbs-plus`, which brings the reference's `bbs_plus` crate in):
//!
//!   `SignatureG1::new(rng, messages, sk, params)`, n times (bbs_plus/src/signature.rs:138-211)   -> `sign_many`, with the caller's `e_i`, `s_i` for the two draws
//!   `sig.verify(messages, pk, params)`, n times (signature.rs:272-296)                            -> `verify_each`: one verdict per signature
//!   the same through `RandomizedPairingChecker`                                                   -> `verify_batch`: one verdict for all
//!   `proof.verify(revealed, challenge, pk, params)`, n times (bbs_plus/src/proof.rs:355-611)      -> `pok_verify_each`: the reference's first error per proof
//!   the same with one verdict for all                                                             -> `pok_verify_batch`
//!
//! `GpuSignatureParams` keeps `[g1, h_0, h ..]` resident on the device and the prepared coefficients of `w` and `g2` beside it: one upload per issuer.
//! Every function answers `None` when the library declines (no device, a bad argument), so that the caller stays on the arkworks path it replaced.
//! NOT compiled in the build image (no Rust toolchain there); `tests/parity.rs` `bbs_plus_bulk_equals_the_reference` and
//! `bbs_plus_pok_bulk_equals_the_reference` compare with the reference's own `new` / `verify` and `PoKOfSignatureG1Proof::verify`.
use crate::ffi::*;
use crate::host::{raw_bbs_plus_pok_verify_batch, raw_bbs_plus_pok_verify_each, raw_bbs_plus_sign_many, raw_bbs_plus_verify_batch, raw_bbs_plus_verify_each};
use crate::{g1_affine, pack_g1, pack_g2, ResidentG1, G2_PREPARED_WORDS};
use ark_bls12_381::{Bls12_381, Fr, G1Affine};
use ark_ec::AffineRepr;
use ark_std::{collections::BTreeMap, vec::Vec};
use bbs_plus::prelude::{BBSPlusError, PoKOfSignatureG1Proof, PublicKeyG2, SecretKey, SignatureG1, SignatureParamsG1};

/// the parameters and the public key of one issuer on the device
pub struct GpuSignatureParams { bases: ResidentG1, l: usize, h_0: Vec<u64>, pk_pc: Vec<u64>, g2_pc: Vec<u64> }
impl GpuSignatureParams {
    /// `None` for parameters without a message generator (`NoMessageToSign`), an identity `w` or `g2`, or when the library declines
    pub fn new(params: &SignatureParamsG1<Bls12_381>, pk: &PublicKeyG2<Bls12_381>) -> Option<Self> {
        let l = params.h.len();
        if l == 0 { return None; }
        let mut pts = Vec::with_capacity(l + 2);
        pts.push(params.g1); pts.push(params.h_0); pts.extend_from_slice(&params.h);
        let (q, qi) = pack_g2(&[pk.0, params.g2]);
        let (mut co, mut inf) = (ark_std::vec![0u64; 2 * G2_PREPARED_WORDS], [0u8; 2]);
        if unsafe { dgpu_g2_prepare(q.as_ptr(), qi.as_ptr(), 2, co.as_mut_ptr(), inf.as_mut_ptr()) } != DGPU_OK || inf != [0u8; 2] { return None; }
        let g2_pc = co.split_off(G2_PREPARED_WORDS);
        let bases = ResidentG1::upload(&pts, None);              // a plain handle: the calls refuse a precomputed table
        if bases.handle() == 0 { return None; }
        Some(GpuSignatureParams { bases, l, h_0: pack_g1(&[params.h_0]).0, pk_pc: co, g2_pc })
    }
    pub fn supported_message_count(&self) -> usize { self.l }
}

// rows of l messages, packed; `None` for a row of another length (`MessageCountIncompatibleWithSigParams`)
fn pack_rows(messages: &[&[Fr]], l: usize) -> Option<Vec<Fr>> {
    let mut flat = Vec::with_capacity(messages.len() * l);
    for m in messages { if m.len() != l { return None; } flat.extend_from_slice(m); }
    Some(flat)
}
fn split(sigs: &[SignatureG1<Bls12_381>]) -> (Vec<u64>, Vec<Fr>, Vec<Fr>) {
    let a: Vec<G1Affine> = sigs.iter().map(|x| x.A).collect();
    (pack_g1(&a).0, sigs.iter().map(|x| x.e).collect(), sigs.iter().map(|x| x.s).collect())      // identity: zero words
}

/// `SignatureG1::new` for every row with `e[i]`, `s[i]` in place of its two draws.  `Some(None)` entries are rows without a signature: `sk + e_i = 0`, where the
/// reference draws `e` again, or an identity `b_i`.
pub fn sign_many(params: &GpuSignatureParams, sk: &SecretKey<Fr>, messages: &[&[Fr]], e: &[Fr], s: &[Fr]) -> Option<Vec<Option<SignatureG1<Bls12_381>>>> {
    let n = messages.len();
    if e.len() != n || s.len() != n { return None; }
    let flat = pack_rows(messages, params.l)?;
    let (mut xy, mut bad) = (ark_std::vec![0u64; n * 12], ark_std::vec![0u8; n]);
    if raw_bbs_plus_sign_many(params.bases.handle(), params.l, &sk.0, &flat, e, s, &mut xy, &mut bad) != DGPU_OK { return None; }
    Some((0..n).map(|i| if bad[i] != 0 { None } else { Some(SignatureG1 { A: g1_affine(xy[12 * i..12 * i + 12].try_into().unwrap(), 0), e: e[i], s: s[i] }) }).collect())
}

/// `sigs[i].verify(messages[i], pk, params).is_ok()` for every i
pub fn verify_each(params: &GpuSignatureParams, sigs: &[SignatureG1<Bls12_381>], messages: &[&[Fr]]) -> Option<Vec<bool>> {
    let n = sigs.len();
    if messages.len() != n { return None; }
    let flat = pack_rows(messages, params.l)?;
    let (a, e, s) = split(sigs);
    let mut ok = ark_std::vec![0u8; n];
    if raw_bbs_plus_verify_each(params.bases.handle(), params.l, &params.pk_pc, &params.g2_pc, &a, &e, &s, &flat, &mut ok) != DGPU_OK { return None; }
    Some(ok.iter().map(|&k| k != 0).collect())
}

/// all of them at once under the weights `random^i` (`random` non-zero); an identity `A` anywhere is a rejection, no signatures at all verify
pub fn verify_batch(params: &GpuSignatureParams, sigs: &[SignatureG1<Bls12_381>], messages: &[&[Fr]], random: &Fr) -> Option<bool> {
    let n = sigs.len();
    if messages.len() != n { return None; }
    if sigs.iter().any(|x| x.A.is_zero()) { return Some(false); }
    let flat = pack_rows(messages, params.l)?;
    let (a, e, s) = split(sigs);
    let mut ok = 0i32;
    if raw_bbs_plus_verify_batch(params.bases.handle(), params.l, &params.pk_pc, &params.g2_pc, &a, &e, &s, &flat, random, &mut ok) != DGPU_OK { return None; }
    Some(ok != 0)
}

// ---- proofs of knowledge of a signature -------------------------------------------------------------------------------------------------------------------
/// the arrays of the C ABI for n proofs: the five points, (z1, z2, z3, z4), the rows of values (the revealed message, or the hidden one's response: from the
/// proof's full response, or from its partial response completed by `missing[i]`, keyed by message index as `verify_partial` takes them) and the masks.
/// `None` where the reference answers with an error that is not one of the four checks (a revealed index out of range, neither or both responses, a response
/// that is missing or of another count).
struct Packed { points: Vec<u64>, fixed: Vec<Fr>, values: Vec<Fr>, revealed: Vec<u8> }
fn pack_proofs(l: usize, proofs: &[PoKOfSignatureG1Proof<Bls12_381>], revealed: &[&BTreeMap<usize, Fr>], missing: Option<&[&BTreeMap<usize, Fr>]>) -> Option<Packed> {
    let n = proofs.len();
    let (mut pts, mut fixed, mut values, mut mask) = (Vec::with_capacity(5 * n), Vec::with_capacity(4 * n), Vec::with_capacity(n * l), ark_std::vec![0u8; n * l]);
    for (i, p) in proofs.iter().enumerate() {
        let rev = revealed[i];
        if rev.keys().any(|&j| j >= l) { return None; }
        let hidden = l - rev.len();
        // the responses of the second protocol in its own order: the hidden messages ascending, then -r3 (over d), then s' (over h_0)
        let resp = |k: usize| -> Option<Fr> {
            match (&p.sc_resp_2, &p.sc_partial_resp_2) {
                (Some(full), None) => if missing.is_some() || full.0.len() != hidden + 2 { None } else { Some(full.0[k]) },
                // (a partial response without missing responses is the reference's MissingResponsesNeededForPartialSchnorrProofVerification, proof.rs:594-596)
                (None, Some(part)) => if missing.is_none() || part.total_responses != hidden + 2 { None } else { part.responses.get(&k).copied() },
                _ => None,
            }
        };
        pts.extend_from_slice(&[p.A_prime, p.A_bar, p.d, p.sc_resp_1.t, p.T2]);
        fixed.extend_from_slice(&[p.sc_resp_1.response1, p.sc_resp_1.response2, resp(hidden)?, resp(hidden + 1)?]);
        let mut k = 0;
        for j in 0..l {
            if let Some(m) = rev.get(&j) { values.push(*m); mask[i * l + j] = 1; continue; }
            let given = missing.and_then(|ms| ms[i].get(&j).copied());
            values.push(match given { Some(z) => z, None => resp(k)? });
            k += 1;
        }
    }
    Some(Packed { points: pack_g1(&pts).0, fixed, values, revealed: mask })      // identity: zero words
}
fn status_to_result(status: u8) -> Result<(), BBSPlusError> {
    match status {
        0 => Ok(()),
        1 => Err(BBSPlusError::ZeroSignature),
        2 => Err(BBSPlusError::FirstSchnorrVerificationFailed),
        3 => Err(BBSPlusError::SecondSchnorrVerificationFailed),
        _ => Err(BBSPlusError::PairingCheckFailed),
    }
}

/// `proofs[i].verify(revealed[i], &challenges[i], pk, params)` for every i (`verify_partial` with `missing[i]` where given): `Ok(())` or the reference's first
/// error among `ZeroSignature`, `FirstSchnorrVerificationFailed`, `SecondSchnorrVerificationFailed`, `PairingCheckFailed`.  The points are taken as validated,
/// as the reference takes them.
pub fn pok_verify_each(params: &GpuSignatureParams, proofs: &[PoKOfSignatureG1Proof<Bls12_381>], revealed: &[&BTreeMap<usize, Fr>], challenges: &[Fr],
                       missing: Option<&[&BTreeMap<usize, Fr>]>) -> Option<Vec<Result<(), BBSPlusError>>> {
    let n = proofs.len();
    if revealed.len() != n || challenges.len() != n || missing.map_or(false, |m| m.len() != n) { return None; }
    let pk = pack_proofs(params.l, proofs, revealed, missing)?;
    let mut status = ark_std::vec![0u8; n];
    if raw_bbs_plus_pok_verify_each(params.bases.handle(), params.l, &params.h_0, &params.pk_pc, &params.g2_pc, &pk.points, &pk.fixed, &pk.values, &pk.revealed, challenges, &mut status)
        != DGPU_OK { return None; }
    Some(status.into_iter().map(status_to_result).collect())
}

/// all of them at once: one G1 equation and one pairing check under the weights `random^(2i)` (first Schnorr check), `random^(2i+1)` (second) and `random^i`
/// (pairing), `random` non-zero; no proofs at all verify.  A batch with a failing proof passes with probability at most 3n / r per equation.
pub fn pok_verify_batch(params: &GpuSignatureParams, proofs: &[PoKOfSignatureG1Proof<Bls12_381>], revealed: &[&BTreeMap<usize, Fr>], challenges: &[Fr],
                        missing: Option<&[&BTreeMap<usize, Fr>]>, random: &Fr) -> Option<bool> {
    let n = proofs.len();
    if revealed.len() != n || challenges.len() != n || missing.map_or(false, |m| m.len() != n) { return None; }
    let pk = pack_proofs(params.l, proofs, revealed, missing)?;
    let mut ok = 0i32;
    if raw_bbs_plus_pok_verify_batch(params.bases.handle(), params.l, &params.h_0, &params.pk_pc, &params.g2_pc, &pk.points, &pk.fixed, &pk.values, &pk.revealed, challenges, random, &mut ok)
        != DGPU_OK { return None; }
    Some(ok != 0)
}

// ---- the 2023 scheme (bbs_plus/src/signature_23.rs, proof_23_cdl.rs, proof_23_ietf.rs): no s, no h_0 ------------------------------------------------------------
//   `Signature23G1::new` / `verify`, n times                                  -> `sign_many_23`, `verify_each_23`, `verify_batch_23`
//   proof_23_cdl's `PoKOfSignature23G1Proof::verify`, n times                 -> `pok_verify_each_23`, `pok_verify_batch_23`
//   proof_23_ietf's `PoKOfSignature23G1Proof::verify`, n times                -> `pok_ietf_verify_each_23`, `pok_ietf_verify_batch_23`
// `GpuSignatureParams23` keeps `[g1, h ..]` resident.  NOT compiled in the build image either; `tests/parity.rs` `bbs23_bulk_equals_the_reference` compares with the
// reference's own `new` / `verify` and both proofs' `verify`.
use crate::host::{raw_bbs23_pok_ietf_verify_batch, raw_bbs23_pok_ietf_verify_each, raw_bbs23_pok_verify_batch, raw_bbs23_pok_verify_each, raw_bbs23_sign_many, raw_bbs23_verify_batch,
                  raw_bbs23_verify_each};
use bbs_plus::proof_23_cdl::PoKOfSignature23G1Proof as CdlProof;
use bbs_plus::proof_23_ietf::PoKOfSignature23G1Proof as IetfProof;
use bbs_plus::setup::SignatureParams23G1;
use bbs_plus::signature_23::Signature23G1;
use schnorr_pok::{partial::PartialSchnorrResponse, SchnorrResponse};

/// the 2023 parameters and the public key of one issuer on the device
pub struct GpuSignatureParams23 { bases: ResidentG1, l: usize, pk_pc: Vec<u64>, g2_pc: Vec<u64> }
impl GpuSignatureParams23 {
    /// `None` for parameters without a message generator, an identity `w` or `g2`, or when the library declines
    pub fn new(params: &SignatureParams23G1<Bls12_381>, pk: &PublicKeyG2<Bls12_381>) -> Option<Self> {
        let l = params.h.len();
        if l == 0 { return None; }
        let mut pts = Vec::with_capacity(l + 1);
        pts.push(params.g1); pts.extend_from_slice(&params.h);
        let (q, qi) = pack_g2(&[pk.0, params.g2]);
        let (mut co, mut inf) = (ark_std::vec![0u64; 2 * G2_PREPARED_WORDS], [0u8; 2]);
        if unsafe { dgpu_g2_prepare(q.as_ptr(), qi.as_ptr(), 2, co.as_mut_ptr(), inf.as_mut_ptr()) } != DGPU_OK || inf != [0u8; 2] { return None; }
        let g2_pc = co.split_off(G2_PREPARED_WORDS);
        let bases = ResidentG1::upload(&pts, None);              // a plain handle: the calls refuse a precomputed table
        if bases.handle() == 0 { return None; }
        Some(GpuSignatureParams23 { bases, l, pk_pc: co, g2_pc })
    }
    pub fn supported_message_count(&self) -> usize { self.l }
}
fn split_23(sigs: &[Signature23G1<Bls12_381>]) -> (Vec<u64>, Vec<Fr>) {
    let a: Vec<G1Affine> = sigs.iter().map(|x| x.A).collect();
    (pack_g1(&a).0, sigs.iter().map(|x| x.e).collect())
}

/// `Signature23G1::new` for every row with `e[i]` in place of its draw.  `None` entries are rows without a signature: `sk + e_i = 0` or an identity `b_i`.
pub fn sign_many_23(params: &GpuSignatureParams23, sk: &SecretKey<Fr>, messages: &[&[Fr]], e: &[Fr]) -> Option<Vec<Option<Signature23G1<Bls12_381>>>> {
    let n = messages.len();
    if e.len() != n { return None; }
    let flat = pack_rows(messages, params.l)?;
    let (mut xy, mut bad) = (ark_std::vec![0u64; n * 12], ark_std::vec![0u8; n]);
    if raw_bbs23_sign_many(params.bases.handle(), params.l, &sk.0, &flat, e, &mut xy, &mut bad) != DGPU_OK { return None; }
    Some((0..n).map(|i| if bad[i] != 0 { None } else { Some(Signature23G1 { A: g1_affine(xy[12 * i..12 * i + 12].try_into().unwrap(), 0), e: e[i] }) }).collect())
}
/// `sigs[i].verify(messages[i], pk, params).is_ok()` for every i
pub fn verify_each_23(params: &GpuSignatureParams23, sigs: &[Signature23G1<Bls12_381>], messages: &[&[Fr]]) -> Option<Vec<bool>> {
    let n = sigs.len();
    if messages.len() != n { return None; }
    let flat = pack_rows(messages, params.l)?;
    let (a, e) = split_23(sigs);
    let mut ok = ark_std::vec![0u8; n];
    if raw_bbs23_verify_each(params.bases.handle(), params.l, &params.pk_pc, &params.g2_pc, &a, &e, &flat, &mut ok) != DGPU_OK { return None; }
    Some(ok.iter().map(|&k| k != 0).collect())
}
/// all of them at once under the weights `random^i` (`random` non-zero); an identity `A` anywhere is a rejection, no signatures at all verify
pub fn verify_batch_23(params: &GpuSignatureParams23, sigs: &[Signature23G1<Bls12_381>], messages: &[&[Fr]], random: &Fr) -> Option<bool> {
    let n = sigs.len();
    if messages.len() != n { return None; }
    if sigs.iter().any(|x| x.A.is_zero()) { return Some(false); }
    let flat = pack_rows(messages, params.l)?;
    let (a, e) = split_23(sigs);
    let mut ok = 0i32;
    if raw_bbs23_verify_batch(params.bases.handle(), params.l, &params.pk_pc, &params.g2_pc, &a, &e, &flat, random, &mut ok) != DGPU_OK { return None; }
    Some(ok != 0)
}

// one proof's row of values and its trailing responses: `tail` responses follow the hidden messages' in the protocol's own order (CDL: the one over d; IETF: the
// two over Abar and Bbar).  `None` where the reference answers with an error that is not one of its checks.
fn pack_row_23(l: usize, i: usize, full: &Option<SchnorrResponse<G1Affine>>, part: &Option<PartialSchnorrResponse<G1Affine>>, tail: usize, rev: &BTreeMap<usize, Fr>,
               missing: Option<&[&BTreeMap<usize, Fr>]>, fixed: &mut Vec<Fr>, values: &mut Vec<Fr>, mask: &mut [u8]) -> Option<()> {
    if rev.keys().any(|&j| j >= l) { return None; }
    let hidden = l - rev.len();
    let resp = |k: usize| -> Option<Fr> {
        match (full, part) {
            (Some(f), None) => if missing.is_some() || f.0.len() != hidden + tail { None } else { Some(f.0[k]) },
            (None, Some(p)) => if missing.is_none() || p.total_responses != hidden + tail { None } else { p.responses.get(&k).copied() },
            _ => None,
        }
    };
    for t in 0..tail { fixed.push(resp(hidden + t)?); }
    let mut k = 0;
    for j in 0..l {
        if let Some(m) = rev.get(&j) { values.push(*m); mask[i * l + j] = 1; continue; }
        let given = missing.and_then(|ms| ms[i].get(&j).copied());
        values.push(match given { Some(z) => z, None => resp(k)? });
        k += 1;
    }
    Some(())
}
fn pack_cdl(l: usize, proofs: &[CdlProof<Bls12_381>], revealed: &[&BTreeMap<usize, Fr>], missing: Option<&[&BTreeMap<usize, Fr>]>) -> Option<Packed> {
    let n = proofs.len();
    let (mut pts, mut fixed, mut values, mut mask) = (Vec::with_capacity(5 * n), Vec::with_capacity(3 * n), Vec::with_capacity(n * l), ark_std::vec![0u8; n * l]);
    for (i, p) in proofs.iter().enumerate() {
        pts.extend_from_slice(&[p.A_bar, p.B_bar, p.d, p.sc_resp_1.t, p.T2]);
        fixed.extend_from_slice(&[p.sc_resp_1.response1, p.sc_resp_1.response2]);
        pack_row_23(l, i, &p.sc_resp_2, &p.sc_partial_resp_2, 1, revealed[i], missing, &mut fixed, &mut values, &mut mask)?;
    }
    Some(Packed { points: pack_g1(&pts).0, fixed, values, revealed: mask })
}
fn pack_ietf(l: usize, proofs: &[IetfProof<Bls12_381>], revealed: &[&BTreeMap<usize, Fr>], missing: Option<&[&BTreeMap<usize, Fr>]>) -> Option<Packed> {
    let n = proofs.len();
    let (mut pts, mut fixed, mut values, mut mask) = (Vec::with_capacity(3 * n), Vec::with_capacity(2 * n), Vec::with_capacity(n * l), ark_std::vec![0u8; n * l]);
    for (i, p) in proofs.iter().enumerate() {
        pts.extend_from_slice(&[p.A_bar, p.B_bar, p.T]);
        pack_row_23(l, i, &p.sc_resp, &p.sc_partial_resp, 2, revealed[i], missing, &mut fixed, &mut values, &mut mask)?;
    }
    Some(Packed { points: pack_g1(&pts).0, fixed, values, revealed: mask })
}
fn counts_ok(n: usize, revealed: &[&BTreeMap<usize, Fr>], challenges: &[Fr], missing: Option<&[&BTreeMap<usize, Fr>]>) -> bool {
    revealed.len() == n && challenges.len() == n && !missing.map_or(false, |m| m.len() != n)
}

/// proof_23_cdl: `proofs[i].verify(revealed[i], &challenges[i], pk, params)` for every i (`verify_partial` with `missing[i]` where given): `Ok(())` or the
/// reference's first error.  The points are taken as validated, as the reference takes them.
pub fn pok_verify_each_23(params: &GpuSignatureParams23, proofs: &[CdlProof<Bls12_381>], revealed: &[&BTreeMap<usize, Fr>], challenges: &[Fr],
                          missing: Option<&[&BTreeMap<usize, Fr>]>) -> Option<Vec<Result<(), BBSPlusError>>> {
    if !counts_ok(proofs.len(), revealed, challenges, missing) { return None; }
    let pk = pack_cdl(params.l, proofs, revealed, missing)?;
    let mut status = ark_std::vec![0u8; proofs.len()];
    if raw_bbs23_pok_verify_each(params.bases.handle(), params.l, &params.pk_pc, &params.g2_pc, &pk.points, &pk.fixed, &pk.values, &pk.revealed, challenges, &mut status) != DGPU_OK {
        return None;
    }
    Some(status.into_iter().map(status_to_result).collect())
}
/// proof_23_cdl, one verdict under the weights `random^(2i)`, `random^(2i+1)`, `random^i` (`random` non-zero); no proofs at all verify
pub fn pok_verify_batch_23(params: &GpuSignatureParams23, proofs: &[CdlProof<Bls12_381>], revealed: &[&BTreeMap<usize, Fr>], challenges: &[Fr],
                           missing: Option<&[&BTreeMap<usize, Fr>]>, random: &Fr) -> Option<bool> {
    if !counts_ok(proofs.len(), revealed, challenges, missing) { return None; }
    let pk = pack_cdl(params.l, proofs, revealed, missing)?;
    let mut ok = 0i32;
    if raw_bbs23_pok_verify_batch(params.bases.handle(), params.l, &params.pk_pc, &params.g2_pc, &pk.points, &pk.fixed, &pk.values, &pk.revealed, challenges, random, &mut ok) != DGPU_OK {
        return None;
    }
    Some(ok != 0)
}
/// proof_23_ietf: as `pok_verify_each_23`; its only Schnorr check fails as `SecondSchnorrVerificationFailed`, the name the reference gives it
pub fn pok_ietf_verify_each_23(params: &GpuSignatureParams23, proofs: &[IetfProof<Bls12_381>], revealed: &[&BTreeMap<usize, Fr>], challenges: &[Fr],
                               missing: Option<&[&BTreeMap<usize, Fr>]>) -> Option<Vec<Result<(), BBSPlusError>>> {
    if !counts_ok(proofs.len(), revealed, challenges, missing) { return None; }
    let pk = pack_ietf(params.l, proofs, revealed, missing)?;
    let mut status = ark_std::vec![0u8; proofs.len()];
    if raw_bbs23_pok_ietf_verify_each(params.bases.handle(), params.l, &params.pk_pc, &params.g2_pc, &pk.points, &pk.fixed, &pk.values, &pk.revealed, challenges, &mut status)
        != DGPU_OK { return None; }
    Some(status.into_iter().map(status_to_result).collect())
}
/// proof_23_ietf, one verdict under the weights `random^i`
pub fn pok_ietf_verify_batch_23(params: &GpuSignatureParams23, proofs: &[IetfProof<Bls12_381>], revealed: &[&BTreeMap<usize, Fr>], challenges: &[Fr],
                                missing: Option<&[&BTreeMap<usize, Fr>]>, random: &Fr) -> Option<bool> {
    if !counts_ok(proofs.len(), revealed, challenges, missing) { return None; }
    let pk = pack_ietf(params.l, proofs, revealed, missing)?;
    let mut ok = 0i32;
    if raw_bbs23_pok_ietf_verify_batch(params.bases.handle(), params.l, &params.pk_pc, &params.g2_pc, &pk.points, &pk.fixed, &pk.values, &pk.revealed, challenges, random, &mut ok)
        != DGPU_OK { return None; }
    Some(ok != 0)
}
