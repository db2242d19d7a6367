//! rust/dock_gpu/src/saver.rs — the reference's `saver` crate (verifiable encryption over LegoGroth16) in bulk (feature `saver`, which brings that crate in):
//!
//!   `PreparedDecryptionKey::pairing_powers(chunk_bit_size, g_i)` (saver/src/keygen.rs:211-234)                  -> `GpuDecryptionKey::new`, `pairing_powers`
//!   `Ciphertext::decrypt_to_chunks_given_pairing_powers(.., sk, ..)`, n times (encryption.rs:569-624)           -> `decrypt_many`
//!   `Ciphertext::verify_decryption(chunks, c_0, c, nu, dk, g_i, gens)`, n times (:425-469)                     -> `verify_decryption_each`
//!   `Ciphertext::verify_ciphertext_commitment(..)`, n times (:367-393)                                         -> `verify_commitment_each`
//!   `Ciphertext::verify_commitments_in_batch(ciphertexts, r_powers, ek, gens)` (:395-422)                      -> `verify_commitments_batch`
//!
//! `GpuDecryptionKey` takes the AFFINE `DecryptionKey` (a `PreparedDecryptionKey` cannot be turned back into points) and keeps the prepared coefficients, the
//! table of GT powers and its search index on the device: one upload and one table build per key.  Every function answers `None` when the library declines (no
//! device, a bad argument), so that the caller stays on the arkworks path it replaced.  NOT compiled in the build image (no Rust toolchain there);
//! `tests/parity.rs` `saver_bulk_equals_the_reference` compares with the reference's own calls.
use crate::ffi::*;
use crate::{fq12_from_words, g1_affine, pack_g1, pack_g2, G2_PREPARED_WORDS};
use ark_bls12_381::{Bls12_381, Fr, G1Affine, G2Affine};
use ark_ec::pairing::PairingOutput;
use ark_std::vec::Vec;
use saver::encryption::Ciphertext;
use saver::error::SaverError;
use saver::keygen::{DecryptionKey, EncryptionKey, SecretKey};      // (chunks are `u16`, the reference's `saver::utils::CHUNK_TYPE`)

// include/dock_gpu_saver.h: served by libdock_gpu_saver.so — the product's objects plus these seven calls — which a host that builds with this feature links
// INSTEAD of libdock_gpu.so (build.rs picks the library by the feature).  Declared here, by hand: ffi.rs is generated from include/dock_gpu.h alone.
extern "C" {
    fn dgpu_saver_dk_create(g_i: *const u64, h: *const u64, v_0: *const u64, v_1: *const u64, v_2: *const u64, chunk_bit_size: i32, k: usize, handle: *mut u64) -> i32;
    fn dgpu_saver_dk_free(dk: u64) -> i32;
    fn dgpu_saver_dk_powers(dk: u64, j: usize, first: usize, count: usize, out: *mut u64) -> i32;
    fn dgpu_saver_decrypt_many(dk: u64, ct: *const u64, n: usize, sk: *const u64, montgomery: i32, chunks: *mut u16, nu_xy: *mut u64, status: *mut u8) -> i32;
    fn dgpu_saver_verify_decryption_each(dk: u64, ct: *const u64, n: usize, chunks: *const u16, nu_xy: *const u64, ok: *mut u8) -> i32;
    fn dgpu_saver_verify_commitment_each(all_pc: *const u64, k: usize, ct: *const u64, n: usize, ok: *mut u8) -> i32;
    fn dgpu_saver_verify_commitments_batch(all_pc: *const u64, k: usize, ct: *const u64, n: usize, r_powers: *const u64, montgomery: i32, ok: *mut i32) -> i32;
}
fn raw_saver_dk_create(g_i: &[u64], h: &[u64; 24], v_0: &[u64; 24], v_1: &[u64], v_2: &[u64], b: u8, k: usize, handle: &mut u64) -> i32 {
    unsafe { dgpu_saver_dk_create(g_i.as_ptr(), h.as_ptr(), v_0.as_ptr(), v_1.as_ptr(), v_2.as_ptr(), b as i32, k, handle) }
}
fn raw_saver_dk_free(dk: u64) -> i32 { unsafe { dgpu_saver_dk_free(dk) } }
fn raw_saver_dk_powers(dk: u64, j: usize, first: usize, count: usize, out: &mut [u64]) -> i32 { unsafe { dgpu_saver_dk_powers(dk, j, first, count, out.as_mut_ptr()) } }
fn raw_saver_decrypt_many(dk: u64, ct: &[u64], sk: &Fr, chunks: &mut [u16], nu: &mut [u64], status: &mut [u8]) -> i32 {
    unsafe { dgpu_saver_decrypt_many(dk, ct.as_ptr(), status.len(), sk as *const Fr as *const u64, 1, chunks.as_mut_ptr(), nu.as_mut_ptr(), status.as_mut_ptr()) }
}
fn raw_saver_verify_decryption_each(dk: u64, ct: &[u64], chunks: &[u16], nu: &[u64], ok: &mut [u8]) -> i32 {
    unsafe { dgpu_saver_verify_decryption_each(dk, ct.as_ptr(), ok.len(), chunks.as_ptr(), nu.as_ptr(), ok.as_mut_ptr()) }
}
fn raw_saver_verify_commitment_each(all_pc: &[u64], k: usize, ct: &[u64], ok: &mut [u8]) -> i32 {
    unsafe { dgpu_saver_verify_commitment_each(all_pc.as_ptr(), k, ct.as_ptr(), ok.len(), ok.as_mut_ptr()) }
}
fn raw_saver_verify_commitments_batch(all_pc: &[u64], k: usize, ct: &[u64], r_powers: &[Fr], ok: &mut i32) -> i32 {
    unsafe { dgpu_saver_verify_commitments_batch(all_pc.as_ptr(), k, ct.as_ptr(), r_powers.len(), r_powers.as_ptr() as *const u64, 1, ok) }
}

/// a decryption key on the device
pub struct GpuDecryptionKey { handle: u64, k: usize, chunk_bit_size: u8 }
impl GpuDecryptionKey {
    /// `None` when the vectors disagree in length, for a chunk size outside 1 ..= 16, more than 255 chunks, or when the library declines (out of memory too)
    pub fn new(dk: &DecryptionKey<Bls12_381>, g_i: &[G1Affine], h: &G2Affine, chunk_bit_size: u8) -> Option<Self> {
        let k = dk.V_1.len();
        if dk.V_2.len() != k || g_i.len() < k { return None; }
        let (g, _) = pack_g1(&g_i[..k]);
        let (hw, _) = pack_g2(core::slice::from_ref(h));
        let (v0, _) = pack_g2(core::slice::from_ref(&dk.V_0));
        let ((v1, _), (v2, _)) = (pack_g2(&dk.V_1), pack_g2(&dk.V_2));
        let mut handle = 0u64;
        if raw_saver_dk_create(&g, hw[..24].try_into().ok()?, v0[..24].try_into().ok()?, &v1, &v2, chunk_bit_size, k, &mut handle) != DGPU_OK { return None; }
        Some(GpuDecryptionKey { handle, k, chunk_bit_size })
    }
    pub fn supported_chunks_count(&self) -> usize { self.k }
    /// the reference's `pairing_powers`: per chunk the `2^chunk_bit_size - 1` powers of `e(g_j, V_2_j)`
    pub fn pairing_powers(&self) -> Option<Vec<Vec<PairingOutput<Bls12_381>>>> {
        let e = (1usize << self.chunk_bit_size) - 1;
        let mut words = ark_std::vec![0u64; e * 72];
        (0..self.k).map(|j| {
            if raw_saver_dk_powers(self.handle, j, 1, e, &mut words) != DGPU_OK { return None; }
            Some(words.chunks(72).map(|w| PairingOutput(fq12_from_words(w.try_into().unwrap()))).collect())
        }).collect()
    }
}
impl Drop for GpuDecryptionKey {
    fn drop(&mut self) { let _ = raw_saver_dk_free(self.handle); }
}

// rows [c_0, c_1 .. c_k, psi]; `None` for a ciphertext of another chunk count (`IncompatibleDecryptionKey` / `IncompatibleEncryptionKey`)
fn pack_rows(cts: &[Ciphertext<Bls12_381>], k: usize) -> Option<Vec<u64>> {
    let mut pts = Vec::with_capacity(cts.len() * (k + 2));
    for c in cts {
        if c.enc_chunks.len() != k { return None; }
        pts.push(c.X_r); pts.extend_from_slice(&c.enc_chunks); pts.push(c.commitment);
    }
    Some(pack_g1(&pts).0)                                        // identity: zero words
}

/// per ciphertext what `decrypt_to_chunks_given_pairing_powers` returns: the chunks and `nu`, or `CouldNotFindDiscreteLog`
pub fn decrypt_many(dk: &GpuDecryptionKey, cts: &[Ciphertext<Bls12_381>], sk: &SecretKey<Fr>) -> Option<Vec<Result<(Vec<u16>, G1Affine), SaverError>>> {
    let (n, k) = (cts.len(), dk.k);
    let rows = pack_rows(cts, k)?;
    let (mut chunks, mut nu, mut status) = (ark_std::vec![0u16; n * k], ark_std::vec![0u64; n * 12], ark_std::vec![0u8; n]);
    if raw_saver_decrypt_many(dk.handle, &rows, &sk.0, &mut chunks, &mut nu, &mut status) != DGPU_OK { return None; }
    Some((0..n).map(|i| {
        if status[i] != 0 { return Err(SaverError::CouldNotFindDiscreteLog); }
        let w = &nu[12 * i..12 * i + 12];
        Ok((chunks[i * k..(i + 1) * k].to_vec(), g1_affine(w.try_into().unwrap(), w.iter().all(|&v| v == 0) as u8)))
    }).collect())
}

/// per ciphertext `verify_decryption`: `true`, or the reference's `InvalidDecryption`
pub fn verify_decryption_each(dk: &GpuDecryptionKey, cts: &[Ciphertext<Bls12_381>], chunks: &[&[u16]], nu: &[G1Affine]) -> Option<Vec<bool>> {
    let (n, k) = (cts.len(), dk.k);
    if chunks.len() != n || nu.len() != n { return None; }
    let rows = pack_rows(cts, k)?;
    let mut flat = Vec::with_capacity(n * k);
    for c in chunks { if c.len() != k { return None; } flat.extend_from_slice(c); }
    let mut ok = ark_std::vec![0u8; n];
    if raw_saver_verify_decryption_each(dk.handle, &rows, &flat, &pack_g1(nu).0, &mut ok) != DGPU_OK { return None; }
    Some(ok.iter().map(|&v| v != 0).collect())
}

/// what the verifier of a presentation holds: the prepared coefficients of `[Z_0 .. Z_k, H]`
pub struct GpuCommitmentKey { all_pc: Vec<u64>, k: usize }
impl GpuCommitmentKey {
    pub fn new(ek: &EncryptionKey<Bls12_381>, h: &G2Affine) -> Option<Self> {
        let k = ek.Z.len().checked_sub(1)?;
        let mut pts = ek.Z.clone(); pts.push(*h);
        let (q, qi) = pack_g2(&pts);
        let (mut co, mut inf) = (ark_std::vec![0u64; (k + 2) * G2_PREPARED_WORDS], ark_std::vec![0u8; k + 2]);
        if unsafe { dgpu_g2_prepare(q.as_ptr(), qi.as_ptr(), k + 2, co.as_mut_ptr(), inf.as_mut_ptr()) } != DGPU_OK { return None; }
        Some(GpuCommitmentKey { all_pc: co, k })
    }
}
/// per ciphertext `verify_ciphertext_commitment`: `true`, or the reference's `InvalidCommitment`
pub fn verify_commitment_each(key: &GpuCommitmentKey, cts: &[Ciphertext<Bls12_381>]) -> Option<Vec<bool>> {
    let rows = pack_rows(cts, key.k)?;
    let mut ok = ark_std::vec![0u8; cts.len()];
    if raw_saver_verify_commitment_each(&key.all_pc, key.k, &rows, &mut ok) != DGPU_OK { return None; }
    Some(ok.iter().map(|&v| v != 0).collect())
}
/// `verify_commitments_in_batch` with the caller's `r_powers`
pub fn verify_commitments_batch(key: &GpuCommitmentKey, cts: &[Ciphertext<Bls12_381>], r_powers: &[Fr]) -> Option<bool> {
    if r_powers.len() != cts.len() { return None; }
    let rows = pack_rows(cts, key.k)?;
    let mut ok = 0i32;
    if raw_saver_verify_commitments_batch(&key.all_pc, key.k, &rows, r_powers, &mut ok) != DGPU_OK { return None; }
    Some(ok != 0)
}
