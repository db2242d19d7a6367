//! rust/dock_gpu/tests/segments_parity.rs — `generic::msm_bigint_segments` (one `dgpu_msm_g*_segments` call) against one arkworks `msm_bigint` per segment
//! (one MI355X visible):
//!
//!   DOCK_GPU_LIB_DIR=<repo>/crypto_amd cargo test --release --test segments_parity
use ark_bls12_381::{Fr, G1Affine, G1Projective, G2Affine, G2Projective};
use ark_ec::{AffineRepr, CurveGroup, VariableBaseMSM};
use ark_ff::{BigInt, PrimeField, UniformRand};
use ark_std::rand::{rngs::StdRng, SeedableRng};
use dock_gpu::*;

fn setup() { assert!(init(0, 1 << 16), "no MI355X / libdock_gpu.so"); unsafe { dgpu_set_min_gpu_n(1); } }
fn g1s(rng: &mut StdRng, n: usize) -> Vec<G1Affine> { G1Projective::normalize_batch(&(0..n).map(|_| G1Projective::rand(rng)).collect::<Vec<_>>()) }
fn g2s(rng: &mut StdRng, n: usize) -> Vec<G2Affine> { G2Projective::normalize_batch(&(0..n).map(|_| G2Projective::rand(rng)).collect::<Vec<_>>()) }
fn bigs(rng: &mut StdRng, n: usize) -> Vec<BigInt<4>> { (0..n).map(|_| Fr::rand(rng).into_bigint()).collect() }

#[test]
fn many_small_msms_each_over_its_own_bases() {
    // ragged segments (empty ones first, last and in a row; one point with an identity base; a multi-block segment), then the SAVER shape: 34 columns of 64
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED5E65);
    for lens in [vec![0usize, 1, 5, 64, 65, 0, 0, 513, 3, 0], vec![64; 34], vec![1; 300]] {
        let mut b1: Vec<Vec<G1Affine>> = lens.iter().map(|&n| g1s(&mut rng, n)).collect();
        let b2: Vec<Vec<G2Affine>> = lens.iter().map(|&n| g2s(&mut rng, n.min(70))).collect();
        let sc: Vec<Vec<BigInt<4>>> = lens.iter().map(|&n| bigs(&mut rng, n)).collect();
        if b1.len() > 3 && b1[3].len() > 2 { b1[3][2] = G1Affine::identity(); }
        let (r1, r2, rs): (Vec<&[G1Affine]>, Vec<&[G2Affine]>, Vec<&[BigInt<4>]>) = (b1.iter().map(|v| &v[..]).collect(), b2.iter().map(|v| &v[..]).collect(), sc.iter().map(|v| &v[..]).collect());
        let got1 = dock_gpu::generic::msm_bigint_segments::<G1Affine>(&r1, &rs);
        let got2 = dock_gpu::generic::msm_bigint_segments::<G2Affine>(&r2, &rs);      // (truncates every pair to its shorter side, as arkworks does)
        assert_eq!((got1.len(), got2.len()), (lens.len(), lens.len()));
        for g in 0..lens.len() {
            assert_eq!(got1[g].into_affine(), G1Projective::msm_bigint(&b1[g], &sc[g]).into_affine(), "G1 segment {} of {:?}", g, lens);
            let k = b2[g].len();
            assert_eq!(got2[g].into_affine(), G2Projective::msm_bigint(&b2[g], &sc[g][..k]).into_affine(), "G2 segment {} of {:?}", g, lens);
        }
    }
    // the raw entry point: identity flags, the empty batch
    let (b, s) = (g1s(&mut rng, 9), bigs(&mut rng, 9));
    let (xy, inf) = pack_g1(&b);
    let seg_end = [4u64, 4, 9];
    let (mut out, mut flags) = (vec![0u64; 3 * 18], vec![7u8; 3]);
    assert_eq!(unsafe { dgpu_msm_g1_segments(xy.as_ptr(), inf.as_ptr(), s.as_ptr() as *const u64, 9, seg_end.as_ptr(), 3, 0, out.as_mut_ptr(), flags.as_mut_ptr()) }, DGPU_OK);
    assert_eq!(flags, vec![0u8, 1, 0]);
    assert_eq!(unsafe { dgpu_msm_g2_segments(core::ptr::null(), core::ptr::null(), core::ptr::null(), 0, core::ptr::null(), 0, 0, core::ptr::null_mut(), core::ptr::null_mut()) }, DGPU_OK);
}
