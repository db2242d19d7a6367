//! rust/dock_gpu/src/coconut.rs — the Pointcheval-Sanders signature of the reference's `coconut-crypto` crate in bulk (feature `coconut`, which brings that
//! crate in):
//!
//!   `Signature::new(rng, messages, sk, params)`, n times (coconut/src/signature/ps_signature.rs:46-64)   -> `sign_many`, with the caller's `r_i` for the draw
//!   `sig.verify(messages, pk, params)`, n times (ps_signature.rs:95-142)                                  -> `verify_each`: one verdict per signature
//!   the same with one verdict for all                                                                     -> `verify_batch`
//!   `pok.verify(challenge, revealed, pk, params)`, n times (proof/signature_pok/proof.rs:32-56)           -> `pok_verify_each`: the reference's error per proof
//!
//! `GpuPsParams` keeps `[alpha_tilde, beta_tilde .., g_tilde]` resident on the device as ONE plain G2 handle, the prepared coefficients of all of them beside
//! it and the window table of `g`: one upload per issuer.  The reference keeps the fields of `Signature` and `SignaturePoK` to its own crate, so both cross as
//! their `CanonicalSerialize` bytes (uncompressed: no square root on either side).  Every function answers `None` when the library declines (no device, a bad
//! argument), so that the caller stays on the arkworks path it replaced.  NOT compiled in the build image (no Rust toolchain there); `tests/parity.rs`
//! `ps_bulk_equals_the_reference` compares with the reference's own `new` / `verify` and `SignaturePoK::verify`.
use crate::ffi::*;
use crate::host::{raw_ps_pok_verify_each, raw_ps_sign_many, raw_ps_verify_batch, raw_ps_verify_each, WindowTableG1};
use crate::{g1_affine, pack_g1, pack_g2, ResidentG2, G2_PREPARED_WORDS};
use ark_bls12_381::{Bls12_381, Fr, G1Affine, G2Affine};
use ark_serialize::{CanonicalDeserialize, CanonicalSerialize};
use ark_std::{collections::BTreeMap, vec::Vec};
use coconut_crypto::setup::{PublicKey, SecretKey, SignatureParams};
use coconut_crypto::{PSError, Signature, SignaturePoK, SignaturePoKError};

/// the parameters and the public key of one issuer on the device
pub struct GpuPsParams { bases: ResidentG2, table: WindowTableG1, l: usize, all_pc: Vec<u64> }
impl GpuPsParams {
    /// `None` for a key without messages (`NoMessages`), an identity among the G2 points or `g`, or when the library declines
    pub fn new(params: &SignatureParams<Bls12_381>, pk: &PublicKey<Bls12_381>) -> Option<Self> {
        let l = pk.beta_tilde.len();
        if l == 0 { return None; }
        let mut pts = Vec::with_capacity(l + 2);
        pts.push(pk.alpha_tilde); pts.extend_from_slice(&pk.beta_tilde); pts.push(params.g_tilde);
        let (q, qi) = pack_g2(&pts);
        let (mut co, mut inf) = (ark_std::vec![0u64; (l + 2) * G2_PREPARED_WORDS], ark_std::vec![0u8; l + 2]);
        if unsafe { dgpu_g2_prepare(q.as_ptr(), qi.as_ptr(), l + 2, co.as_mut_ptr(), inf.as_mut_ptr()) } != DGPU_OK || inf.iter().any(|&k| k != 0) { return None; }
        let bases = ResidentG2::upload(&pts, None);              // a plain handle: the calls refuse a precomputed table
        if bases.handle() == 0 { return None; }
        Some(GpuPsParams { bases, table: WindowTableG1::new(&params.g)?, l, all_pc: co })
    }
    pub fn supported_message_count(&self) -> usize { self.l }
    fn g_tilde_pc(&self) -> &[u64] { &self.all_pc[(self.l + 1) * G2_PREPARED_WORDS..] }
}

// rows of l messages, packed; `None` for a row of another length (`InvalidMessageCount`)
fn pack_rows(messages: &[&[Fr]], l: usize) -> Option<Vec<Fr>> {
    let mut flat = Vec::with_capacity(messages.len() * l);
    for m in messages { if m.len() != l { return None; } flat.extend_from_slice(m); }
    Some(flat)
}
// (sigma_1, sigma_2) of a signature through its bytes
fn split(sig: &Signature<Bls12_381>) -> Option<(G1Affine, G1Affine)> {
    let mut bytes = Vec::new();
    sig.serialize_uncompressed(&mut bytes).ok()?;
    <(G1Affine, G1Affine)>::deserialize_uncompressed_unchecked(&bytes[..]).ok()
}
fn combine(sigma_1: G1Affine, sigma_2: G1Affine) -> Option<Signature<Bls12_381>> {
    let mut bytes = Vec::new();
    (sigma_1, sigma_2).serialize_uncompressed(&mut bytes).ok()?;
    Signature::deserialize_uncompressed_unchecked(&bytes[..]).ok()
}
fn pack_sigs(sigs: &[Signature<Bls12_381>]) -> Option<Vec<u64>> {
    let mut pts = Vec::with_capacity(2 * sigs.len());
    for s in sigs { let (a, b) = split(s)?; pts.push(a); pts.push(b); }
    Some(pack_g1(&pts).0)                                        // identity: zero words
}

/// `Signature::new` for every row with `r[i]` in place of its draw.  An entry whose `is_zero()` holds (`r_i = 0`, or `x + sum_j y_j m_ij = 0`) is what the
/// reference returns there too; every verifier refuses it.
pub fn sign_many(params: &GpuPsParams, sk: &SecretKey<Fr>, messages: &[&[Fr]], r: &[Fr]) -> Option<Vec<Signature<Bls12_381>>> {
    let n = messages.len();
    if r.len() != n || sk.y.len() != params.l { return None; }
    let flat = pack_rows(messages, params.l)?;
    let mut key = Vec::with_capacity(params.l + 1);
    key.push(sk.x); key.extend_from_slice(&sk.y);
    let (mut xy, mut bad) = (ark_std::vec![0u64; n * 24], ark_std::vec![0u8; n]);
    let rc = raw_ps_sign_many(params.table.raw_handle(), params.l, &key, &flat, r, &mut xy, &mut bad);
    for k in key.iter_mut() { *k = Fr::from(0u64); }           // (the copy of the secret key made here)
    if rc != DGPU_OK { return None; }
    let point = |w: &[u64]| g1_affine(w.try_into().unwrap(), w.iter().all(|&v| v == 0) as u8);
    (0..n).map(|i| combine(point(&xy[24 * i..24 * i + 12]), point(&xy[24 * i + 12..24 * i + 24]))).collect()
}

/// `sigs[i].verify(messages[i], pk, params).is_ok()` for every i
pub fn verify_each(params: &GpuPsParams, sigs: &[Signature<Bls12_381>], messages: &[&[Fr]]) -> Option<Vec<bool>> {
    let n = sigs.len();
    if messages.len() != n { return None; }
    let flat = pack_rows(messages, params.l)?;
    let a = pack_sigs(sigs)?;
    let mut ok = ark_std::vec![0u8; n];
    if raw_ps_verify_each(params.bases.handle(), params.l, params.g_tilde_pc(), &a, &flat, &mut ok) != DGPU_OK { return None; }
    Some(ok.iter().map(|&k| k != 0).collect())
}

/// all of them at once under the weights `random^i` (`random` non-zero); an identity element anywhere is a rejection, no signatures at all verify
pub fn verify_batch(params: &GpuPsParams, sigs: &[Signature<Bls12_381>], messages: &[&[Fr]], random: &Fr) -> Option<bool> {
    let n = sigs.len();
    if messages.len() != n { return None; }
    if sigs.iter().any(|s| s.is_zero()) { return Some(false); }
    let flat = pack_rows(messages, params.l)?;
    let a = pack_sigs(sigs)?;
    let mut ok = 0i32;
    if raw_ps_verify_batch(params.bases.handle(), params.l, &params.all_pc, &a, n, &flat, random, &mut ok) != DGPU_OK { return None; }
    Some(ok != 0)
}

// the fields of a `SignaturePoK` in the order it serializes them: `k: WithSchnorrResponse { commitment, response, committed_message_indices, value }`, then
// `randomized_sig` (proof.rs:22-26, with_schnorr_response.rs:24-30)
struct PokFields { t: G2Affine, responses: Vec<Fr>, k: G2Affine, sigma: (G1Affine, G1Affine) }
fn pok_fields(p: &SignaturePoK<Bls12_381>) -> Option<PokFields> {
    let mut bytes = Vec::new();
    p.serialize_uncompressed(&mut bytes).ok()?;
    let mut rd = &bytes[..];
    let t = G2Affine::deserialize_uncompressed_unchecked(&mut rd).ok()?;
    let responses = Vec::<Fr>::deserialize_uncompressed_unchecked(&mut rd).ok()?;
    let (_start, _end) = (u64::deserialize_uncompressed_unchecked(&mut rd).ok()?, u64::deserialize_uncompressed_unchecked(&mut rd).ok()?);
    let k = G2Affine::deserialize_uncompressed_unchecked(&mut rd).ok()?;
    let sigma = <(G1Affine, G1Affine)>::deserialize_uncompressed_unchecked(&mut rd).ok()?;
    Some(PokFields { t, responses, k, sigma })
}
fn status_to_result(status: u8) -> Result<(), SignaturePoKError> {
    match status {
        0 => Ok(()),
        1 => Err(SignaturePoKError::SignatureError(PSError::ZeroSignature)),
        3 => Err(SignaturePoKError::SchnorrError(schnorr_pok::error::SchnorrError::InvalidResponse)),
        _ => Err(SignaturePoKError::SignatureError(PSError::PairingCheckFailed)),
    }
}

/// `proofs[i].verify(&challenges[i], revealed[i], pk, params)` for every i: `Ok(())`, or the reference's error in the order it returns them — the Schnorr
/// check's, then `ZeroSignature`, then `PairingCheckFailed` (proof.rs:46-55).  `revealed[i]`: message index -> message, as the reference's sorted iterator yields
/// them.  `None` where the reference answers with an error that is not one of these (a revealed index out of range, a response count that does not fit).
pub fn pok_verify_each(params: &GpuPsParams, proofs: &[SignaturePoK<Bls12_381>], revealed: &[&BTreeMap<usize, Fr>], challenges: &[Fr])
                       -> Option<Vec<Result<(), SignaturePoKError>>> {
    let (n, l) = (proofs.len(), params.l);
    if revealed.len() != n || challenges.len() != n { return None; }
    let (mut sig, mut g2, mut resp_r, mut values, mut mask) = (Vec::with_capacity(2 * n), Vec::with_capacity(2 * n), Vec::with_capacity(n), Vec::with_capacity(n * l), ark_std::vec![0u8; n * l]);
    for (i, p) in proofs.iter().enumerate() {
        let f = pok_fields(p)?;
        let rev = revealed[i];
        if rev.keys().any(|&j| j >= l) || f.responses.len() != l - rev.len() + 1 { return None; }
        let mut k = 0;
        for j in 0..l {
            if let Some(m) = rev.get(&j) { values.push(*m); mask[i * l + j] = 1; } else { values.push(f.responses[k]); k += 1; }
        }
        resp_r.push(f.responses[k]);
        sig.push(f.sigma.0); sig.push(f.sigma.1); g2.push(f.k); g2.push(f.t);
    }
    let mut status = ark_std::vec![0u8; n];
    if raw_ps_pok_verify_each(params.bases.handle(), l, params.g_tilde_pc(), &pack_g1(&sig).0, &pack_g2(&g2).0, &resp_r, &values, &mask, challenges, &mut status) != DGPU_OK {
        return None;
    }
    Some(status.into_iter().map(status_to_result).collect())
}
