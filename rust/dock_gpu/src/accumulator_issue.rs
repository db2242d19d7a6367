//! rust/dock_gpu/src/accumulator_issue.rs — the accumulator manager ISSUING witnesses (the update half lives in host.rs):
//!
//!   `UniversalAccumulator::compute_d_for_batch_given_members(non_members, members)` (vb_accumulator/src/universal.rs:479-495)   -> `d_for_batch`
//!   the same with the member set resident on the device, one upload for every batch and partition                                  -> `ResidentMembers::d_for_batch`
//!   `...::compute_non_membership_witnesses_for_batch_given_d(d, non_members, sk, params_gen)` (universal.rs:499-535)              -> `non_membership_witnesses`
//!   `PositiveAccumulator::compute_membership_witnesses_for_batch(members, sk)` (vb_accumulator/src/positive.rs:369-381)           -> `membership_witnesses`
//!
//! Every function answers `None` when the library declines (no device, a bad argument), so that the caller stays on the arkworks path it replaced;
//! a zero `d` is the reference's `Err(CannotBeZero)` for the whole batch (universal.rs:506-508): `Some(Err(CannotBeZero))`.
//! NOT compiled in the build image (no Rust toolchain there); `tests/parity_accumulator_issue.rs` has a case per function.
use crate::ffi::*;
use crate::g1_affine;
use crate::host::{raw_accumulator_d_for_batch, raw_accumulator_d_for_batch_resident, raw_accumulator_membership_witnesses, raw_accumulator_non_membership_witnesses};
use ark_bls12_381::{Fr, G1Affine};
use ark_std::vec::Vec;

/// the reference's `VBAccumulatorError::CannotBeZero`: some `d_i` is zero, i.e. a "non-member" is a member
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct CannotBeZero;

fn points(xy: &[u64], inf: &[u8]) -> Vec<G1Affine> { (0..inf.len()).map(|i| g1_affine(xy[12 * i..12 * i + 12].try_into().unwrap(), inf[i])).collect() }

/// `d_i = d_in_i prod_j (members_j - non_members_i)`; `d_in = None` is one.  Feeding the result for one partition of the members as the `d_in` of the next is the
/// reference's "partition the members, multiply the outputs" (universal.rs:476-478).  A zero entry marks a non-member that is a member.
pub fn d_for_batch(non_members: &[Fr], members: &[Fr], d_in: Option<&[Fr]>) -> Option<Vec<Fr>> {
    let m = non_members.len();
    let din = d_in.unwrap_or(&[]);
    if d_in.is_some() && din.len() != m { return None; }
    let (mut d, mut nz) = (ark_std::vec![Fr::from(0u64); m], ark_std::vec![0u8; m]);
    if raw_accumulator_d_for_batch(members, non_members, din, &mut d, &mut nz) != DGPU_OK { return None; }
    Some(d)
}

/// the members of an accumulator resident on the device (32 bytes each): uploaded once, read by every `d_for_batch` after
pub struct ResidentMembers { handle: u64, len: usize }
impl ResidentMembers {
    pub fn new(members: &[Fr]) -> Option<Self> {
        let mut handle = 0u64;
        if unsafe { dgpu_scalars_upload(members.as_ptr() as *const u64, members.len(), 1, &mut handle) } != DGPU_OK { return None; }
        Some(ResidentMembers { handle, len: members.len() })
    }
    pub fn len(&self) -> usize { self.len }
    pub fn is_empty(&self) -> bool { self.len == 0 }
    /// `d_for_batch` over the members `[offset, offset + n)` of the resident set
    pub fn d_for_batch(&self, non_members: &[Fr], offset: usize, n: usize, d_in: Option<&[Fr]>) -> Option<Vec<Fr>> {
        let m = non_members.len();
        let din = d_in.unwrap_or(&[]);
        if (d_in.is_some() && din.len() != m) || offset > self.len || n > self.len - offset { return None; }
        let (mut d, mut nz) = (ark_std::vec![Fr::from(0u64); m], ark_std::vec![0u8; m]);
        if raw_accumulator_d_for_batch_resident(self.handle, offset, n, non_members, din, &mut d, &mut nz) != DGPU_OK { return None; }
        Some(d)
    }
}
impl Drop for ResidentMembers { fn drop(&mut self) { unsafe { dgpu_scalars_free(self.handle); } } }

/// `C_i = ((f_V - d_i) / (y_i + alpha)) params_gen`, normalised; `Some(Err(CannotBeZero))` when any `d_i` is zero, as the reference answers
pub fn non_membership_witnesses(d: &[Fr], non_members: &[Fr], f_v: &Fr, alpha: &Fr, params_gen: &G1Affine) -> Option<Result<Vec<G1Affine>, CannotBeZero>> {
    let m = non_members.len();
    if d.len() != m { return None; }
    let (mut xy, mut inf, mut ok) = (ark_std::vec![0u64; m * 12], ark_std::vec![0u8; m], ark_std::vec![0u8; m]);
    if raw_accumulator_non_membership_witnesses(d, non_members, f_v, alpha, params_gen, &mut xy, &mut inf, &mut ok) != DGPU_OK { return None; }
    if ok.iter().any(|&k| k == 0) { return Some(Err(CannotBeZero)); }
    Some(Ok(points(&xy, &inf)))
}

/// `C_i = (1 / (y_i + alpha)) V`, normalised
pub fn membership_witnesses(members: &[Fr], alpha: &Fr, accumulator: &G1Affine) -> Option<Vec<G1Affine>> {
    let m = members.len();
    let (mut xy, mut inf) = (ark_std::vec![0u64; m * 12], ark_std::vec![0u8; m]);
    if raw_accumulator_membership_witnesses(members, alpha, accumulator, &mut xy, &mut inf) != DGPU_OK { return None; }
    Some(points(&xy, &inf))
}
