//! rust/dock_gpu/tests/encode_parity.rs — src/encode.rs against arkworks' `CanonicalSerialize` (one MI355X visible):
//!
//!   DOCK_GPU_LIB_DIR=<repo>/crypto_amd cargo test --release --test encode_parity
use ark_bls12_381::{G1Affine, G1Projective, G2Affine, G2Projective};
use ark_ec::{AffineRepr, CurveGroup};
use ark_serialize::CanonicalSerialize;
use ark_std::rand::{rngs::StdRng, SeedableRng};
use ark_std::UniformRand;
use dock_gpu::*;

fn setup() { assert!(init(0, 1 << 16), "no MI355X / libdock_gpu.so"); }
fn bytes<P: CanonicalSerialize>(ps: &[P], compressed: bool) -> Vec<u8> {
    let mut e = Vec::new();
    for p in ps { if compressed { p.serialize_compressed(&mut e).unwrap() } else { p.serialize_uncompressed(&mut e).unwrap() } }
    e
}

#[test]
fn device_encoding_equals_arkworks() {
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED00E7);
    let mut b1: Vec<G1Affine> = G1Projective::normalize_batch(&(0..1000).map(|_| G1Projective::rand(&mut rng)).collect::<Vec<_>>());
    let mut b2: Vec<G2Affine> = G2Projective::normalize_batch(&(0..200).map(|_| G2Projective::rand(&mut rng)).collect::<Vec<_>>());
    b1[7] = G1Affine::identity(); b2[3] = G2Affine::identity();
    let neg1: Vec<G1Affine> = b1.iter().map(|p| -*p).collect();
    b1.extend(neg1);
    for compressed in [true, false] {
        let (e1, e2) = (bytes(&b1, compressed), bytes(&b2, compressed));
        assert_eq!(serialize_g1_device(&b1, compressed).unwrap(), e1);
        assert_eq!(serialize_g2_device(&b2, compressed).unwrap(), e2);
        // resident bases: plain, then as a precomputed table, whole and in ranges
        for bits in [None, Some(16)] {
            let (r1, r2) = (ResidentG1::upload(&b1, bits), ResidentG2::upload(&b2, bits));
            assert_eq!(bases_serialize_g1(r1.handle(), 0, b1.len(), compressed).unwrap(), e1);
            assert_eq!(bases_serialize_g2(r2.handle(), 0, b2.len(), compressed).unwrap(), e2);
            let sz = e1.len() / b1.len();
            assert_eq!(bases_serialize_g1(r1.handle(), 5, 300, compressed).unwrap(), e1[5 * sz..305 * sz].to_vec());
            let w1 = bases_read_g1(r1.handle(), 0, b1.len()).unwrap();
            assert_eq!(w1, pack_g1(&b1).0.chunks(12).map(|c| <[u64; 12]>::try_from(c).unwrap()).collect::<Vec<_>>());
            let w2 = bases_read_g2(r2.handle(), 0, b2.len()).unwrap();
            assert_eq!(w2, pack_g2(&b2).0.chunks(24).map(|c| <[u64; 24]>::try_from(c).unwrap()).collect::<Vec<_>>());
            assert!(bases_read_g1(r2.handle(), 0, 1).is_none() && bases_serialize_g2(r1.handle(), 0, 1, compressed).is_none());
            assert!(bases_read_g1(r1.handle(), b1.len(), 1).is_none());
        }
    }
}
