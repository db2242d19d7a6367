//! rust/dock_gpu/src/bpp_range_proof.rs — the VERIFIER of the reference's `bulletproofs_plus_plus` crate in bulk (feature `bulletproofs-plus-plus`, which brings
//! that crate in): BoundCheckBpp's proof, for n proofs of ONE shape (base, num_bits, values a proof) over ONE `SetupParams`
//!
//!   `proof.verify(num_bits, &V, &setup_params, &mut transcript)`, n times (`Proof`, range_proof.rs:773-873)   -> `verify_each`
//!   one verdict for all under the weights `random^i`                                                         -> `verify_batch`
//!   the challenges the reference's verifier would draw (range_proof.rs:86-131, weighted_norm_linear_argument.rs:413-418)   -> `challenges`
//!
//! `GpuSetup` keeps `[G, H_vec, G_vec]` resident: one upload per setup.  `Proof`'s fields are private, so `Parts` reads a proof through its own
//! `CanonicalSerialize` image: base, D, M, R, S, then the argument's X, R, l, n.  The challenges are inputs of the calls, as in `proof_system`, whose transcript is
//! shared with the presentation's other statements.  Every function answers `None` when the library declines (no device, a bad argument, an argument whose l or
//! n is longer than one element), so that the caller stays on the arkworks path it replaced.  NOT compiled in the build image (no Rust toolchain there);
//! `tests/parity.rs` `bpp_range_proofs_bulk_equal_the_reference` compares with the reference's own `verify`.
use crate::ffi::*;
use crate::pack_g1;
use ark_bls12_381::{Fr, G1Affine};
use ark_serialize::{CanonicalDeserialize, CanonicalSerialize};
use ark_std::vec::Vec;
use bulletproofs_plus_plus::range_proof::Proof;
use bulletproofs_plus_plus::setup::SetupParams;
use dock_crypto_utils::transcript::Transcript;

// include/dock_gpu_bpp.h: served by libdock_gpu_bpp.so — the product's objects plus these two calls — which a host that builds with this feature links INSTEAD
// of libdock_gpu.so (build.rs picks the library by the feature).  Declared here, by hand: ffi.rs is generated from include/dock_gpu.h alone.
extern "C" {
    fn dgpu_bpp_range_proofs_verify_each_g1(setup: u64, base: u32, num_bits: u32, m: u32, values: *const u64, round_points: *const u64, wnla_points: *const u64, l_n: *const u64,
                                            challenges: *const u64, n: usize, montgomery: i32, status: *mut u8) -> i32;
    fn dgpu_bpp_range_proofs_verify_batch_g1(setup: u64, base: u32, num_bits: u32, m: u32, values: *const u64, round_points: *const u64, wnla_points: *const u64, l_n: *const u64,
                                             challenges: *const u64, n: usize, montgomery: i32, random: *const u64, ok: *mut i32) -> i32;
}

/// `SetupParams` on the device: a plain G1 bases handle `[G, H_0 .. H_7, G_0 ..]`
pub struct GpuSetup { handle: u64, n_g: usize }
impl GpuSetup {
    /// `None` unless H_vec holds 8 points and no generator is the identity, or when the library declines
    pub fn new(setup: &SetupParams<G1Affine>) -> Option<Self> {
        if setup.H_vec.len() != 8 { return None; }
        let mut pts = ark_std::vec![setup.G];
        pts.extend_from_slice(&setup.H_vec);
        pts.extend_from_slice(&setup.G_vec);
        let (xy, inf) = pack_g1(&pts);
        if inf.iter().any(|&f| f != 0) { return None; }
        let mut handle = 0u64;
        if unsafe { dgpu_bases_upload_g1(xy.as_ptr(), core::ptr::null(), pts.len(), &mut handle) } != DGPU_OK { return None; }
        Some(GpuSetup { handle, n_g: setup.G_vec.len() })
    }
}
impl Drop for GpuSetup {
    fn drop(&mut self) { unsafe { dgpu_bases_free(self.handle); } }
}

/// what a proof holds, read from its serialized image
pub struct Parts { pub base: u16, pub round: [G1Affine; 4], pub x: Vec<G1Affine>, pub r: Vec<G1Affine>, pub l: Vec<Fr>, pub n: Vec<Fr> }
impl Parts {
    pub fn of(proof: &Proof<G1Affine>) -> Option<Self> {
        let mut bytes = Vec::new();
        proof.serialize_compressed(&mut bytes).ok()?;
        let mut rd = &bytes[..];
        let base = u16::deserialize_compressed(&mut rd).ok()?;
        let mut round = [G1Affine::default(); 4];
        for p in round.iter_mut() { *p = G1Affine::deserialize_compressed(&mut rd).ok()?; }       // D, M, R, S
        let x = Vec::<G1Affine>::deserialize_compressed(&mut rd).ok()?;
        let r = Vec::<G1Affine>::deserialize_compressed(&mut rd).ok()?;
        let l = Vec::<Fr>::deserialize_compressed(&mut rd).ok()?;
        let n = Vec::<Fr>::deserialize_compressed(&mut rd).ok()?;
        Some(Parts { base, round, x, r, l, n })
    }
}

/// NG and K of a shape, or `None` for a shape the calls refuse
pub fn shape(base: u16, num_bits: u16, m: usize) -> Option<(usize, usize)> {
    if ![2u16, 4, 8, 16].contains(&base) || !num_bits.is_power_of_two() || num_bits > 64 || !m.is_power_of_two() || m > 8 { return None; }
    let bb = base.trailing_zeros() as u16;
    if num_bits < bb { return None; }
    let ng = core::cmp::max((num_bits / bb) as usize, base as usize) * m;
    if !ng.is_power_of_two() { return None; }
    Some((ng, core::cmp::max(3, ng.trailing_zeros() as usize)))
}

/// [e, x, y, r, lambda, delta, t, gamma_0 ..] in the order the calls take them, from the transcript in the state the reference's verifier would find it in
pub fn challenges(transcript: &mut impl Transcript, num_bits: u16, v: &[G1Affine], p: &Parts) -> Vec<Fr> {
    transcript.append_message(b"base", &p.base.to_le_bytes());
    transcript.append_message(b"num_bits", &num_bits.to_le_bytes());
    for v_i in v { transcript.append(b"V", v_i); }
    transcript.append(b"D", &p.round[0]);
    transcript.append(b"M", &p.round[1]);
    let mut out = ark_std::vec![transcript.challenge_scalar::<Fr>(b"e")];
    transcript.append(b"R", &p.round[2]);
    for label in [&b"x"[..], b"y", b"r", b"lambda", b"delta"] { out.push(transcript.challenge_scalar::<Fr>(label)); }
    transcript.append(b"S", &p.round[3]);
    out.push(transcript.challenge_scalar::<Fr>(b"t"));
    for (x, r) in p.x.iter().zip(&p.r) {
        transcript.append(b"X", x);
        transcript.append(b"R", r);
        out.push(transcript.challenge_scalar::<Fr>(b"gamma"));
    }
    out
}

struct Packed { values: Vec<u64>, round: Vec<u64>, wnla: Vec<u64>, l_n: Vec<Fr>, chal: Vec<Fr>, base: u16, m: usize }
fn pack(setup: &GpuSetup, num_bits: u16, vs: &[Vec<G1Affine>], parts: &[Parts], chals: &[Vec<Fr>]) -> Option<Packed> {
    let n = parts.len();
    if n == 0 || vs.len() != n || chals.len() != n { return None; }
    let (base, m) = (parts[0].base, vs[0].len());
    let (ng, k) = shape(base, num_bits, m)?;
    if ng != setup.n_g { return None; }
    let mut o = Packed { values: Vec::new(), round: Vec::new(), wnla: Vec::new(), l_n: Vec::new(), chal: Vec::new(), base, m };
    for i in 0..n {
        let p = &parts[i];
        if p.base != base || vs[i].len() != m || p.x.len() != k || p.r.len() != k || p.l.len() != 1 || p.n.len() != 1 || chals[i].len() != 7 + k { return None; }
        o.values.extend(pack_g1(&vs[i]).0);
        o.round.extend(pack_g1(&p.round).0);
        o.wnla.extend(pack_g1(&p.x).0);
        o.wnla.extend(pack_g1(&p.r).0);
        o.l_n.push(p.l[0]); o.l_n.push(p.n[0]);
        o.chal.extend_from_slice(&chals[i]);
    }
    Some(o)
}

/// per proof `Ok(())`, `Err(1)` (WeightedNormLinearArgumentVerificationFailed) or `Err(2)` (an inverse the reference unwrap()s does not exist)
pub fn verify_each(setup: &GpuSetup, num_bits: u16, vs: &[Vec<G1Affine>], parts: &[Parts], chals: &[Vec<Fr>]) -> Option<Vec<Result<(), u8>>> {
    if parts.is_empty() { return Some(Vec::new()); }
    let o = pack(setup, num_bits, vs, parts, chals)?;
    let mut status = ark_std::vec![0u8; parts.len()];
    // the `&[Fr]` slices go over as they are (Montgomery limbs): montgomery = 1
    let rc = unsafe { dgpu_bpp_range_proofs_verify_each_g1(setup.handle, o.base as u32, num_bits as u32, o.m as u32, o.values.as_ptr(), o.round.as_ptr(), o.wnla.as_ptr(),
                                                           o.l_n.as_ptr() as *const u64, o.chal.as_ptr() as *const u64, parts.len(), 1, status.as_mut_ptr()) };
    if rc != DGPU_OK { return None; }
    Some(status.into_iter().map(|s| if s == 0 { Ok(()) } else { Err(s) }).collect())
}

/// one verdict: proof i weighed by `random^i` (`random` non-zero, from the verifier's own randomness)
pub fn verify_batch(setup: &GpuSetup, num_bits: u16, vs: &[Vec<G1Affine>], parts: &[Parts], chals: &[Vec<Fr>], random: &Fr) -> Option<bool> {
    if parts.is_empty() { return Some(true); }
    let o = pack(setup, num_bits, vs, parts, chals)?;
    let mut ok = 0i32;
    let rc = unsafe { dgpu_bpp_range_proofs_verify_batch_g1(setup.handle, o.base as u32, num_bits as u32, o.m as u32, o.values.as_ptr(), o.round.as_ptr(), o.wnla.as_ptr(),
                                                            o.l_n.as_ptr() as *const u64, o.chal.as_ptr() as *const u64, parts.len(), 1, random as *const Fr as *const u64, &mut ok) };
    if rc != DGPU_OK { return None; }
    Some(ok == 1)
}
