//! rust/dock_gpu/src/encode.rs — `CanonicalSerialize` bytes made on the device, and resident bases read back (include/dock_gpu.h:
//! dgpu_g*_serialize_device, dgpu_bases_read_g*, dgpu_bases_serialize_g*).  The calls sit in src/host.rs beside the rest of the (de)serialisation;
//! this module gives them their public names.  Cases against arkworks: tests/encode_parity.rs.
use ark_bls12_381::{G1Affine, G2Affine};
use ark_std::vec::Vec;

/// serialize_g1 encoded on the current device (the same bytes); None: no device or another error
pub fn serialize_g1_device(points: &[G1Affine], compressed: bool) -> Option<Vec<u8>> { crate::host::device_serialize_g1(points, compressed) }
/// serialize_g2 encoded on the current device (the same bytes)
pub fn serialize_g2_device(points: &[G2Affine], compressed: bool) -> Option<Vec<u8>> { crate::host::device_serialize_g2(points, compressed) }
/// the affine ABI words of points [offset, offset + n) of a G1 bases handle (plain, precomputed table or sharded set); an identity is all-zero words.
/// None: not a G1 bases handle, a range past its end, or another error
pub fn bases_read_g1(handle: u64, offset: usize, n: usize) -> Option<Vec<[u64; 12]>> { crate::host::handle_read_g1(handle, offset, n) }
/// bases_read_g1 for a G2 bases handle
pub fn bases_read_g2(handle: u64, offset: usize, n: usize) -> Option<Vec<[u64; 24]>> { crate::host::handle_read_g2(handle, offset, n) }
/// `CanonicalSerialize` of points [offset, offset + n) of a G1 bases handle, encoded on the device that holds it
pub fn bases_serialize_g1(handle: u64, offset: usize, n: usize, compressed: bool) -> Option<Vec<u8>> { crate::host::handle_serialize_g1(handle, offset, n, compressed) }
/// bases_serialize_g1 for a G2 bases handle
pub fn bases_serialize_g2(handle: u64, offset: usize, n: usize, compressed: bool) -> Option<Vec<u8>> { crate::host::handle_serialize_g2(handle, offset, n, compressed) }
