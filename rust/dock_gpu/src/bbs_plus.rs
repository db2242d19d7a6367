//! rust/dock_gpu/src/bbs_plus.rs — the plain G1 BBS+ signature in bulk (feature `bbs-plus`, which brings the reference's `bbs_plus` crate in):
//!
//!   `SignatureG1::new(rng, messages, sk, params)`, n times (bbs_plus/src/signature.rs:138-211)   -> `sign_many`, with the caller's `e_i`, `s_i` for the two draws
//!   `sig.verify(messages, pk, params)`, n times (signature.rs:272-296)                            -> `verify_each`: one verdict per signature
//!   the same through `RandomizedPairingChecker`                                                   -> `verify_batch`: one verdict for all
//!
//! `GpuSignatureParams` keeps `[g1, h_0, h ..]` resident on the device and the prepared coefficients of `w` and `g2` beside it: one upload per issuer.
//! Every function answers `None` when the library declines (no device, a bad argument), so that the caller stays on the arkworks path it replaced.
//! NOT compiled in the build image (no Rust toolchain there); `tests/parity.rs` `bbs_plus_bulk_equals_the_reference` compares with the reference's own
//! `new` / `verify`.
use crate::ffi::*;
use crate::host::{raw_bbs_plus_sign_many, raw_bbs_plus_verify_batch, raw_bbs_plus_verify_each};
use crate::{g1_affine, pack_g1, pack_g2, ResidentG1, G2_PREPARED_WORDS};
use ark_bls12_381::{Bls12_381, Fr, G1Affine};
use ark_ec::AffineRepr;
use ark_std::vec::Vec;
use bbs_plus::prelude::{PublicKeyG2, SecretKey, SignatureG1, SignatureParamsG1};

/// the parameters and the public key of one issuer on the device
pub struct GpuSignatureParams { bases: ResidentG1, l: usize, pk_pc: Vec<u64>, g2_pc: Vec<u64> }
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
        Some(GpuSignatureParams { bases, l, pk_pc: co, g2_pc })
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
