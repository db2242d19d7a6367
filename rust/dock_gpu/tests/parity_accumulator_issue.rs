//! rust/dock_gpu/tests/parity_accumulator_issue.rs — src/accumulator_issue.rs against the reference's arithmetic done with arkworks (one MI355X visible):
//! compute_d_for_batch_given_members (vb_accumulator/src/universal.rs:479-495), compute_non_membership_witnesses_for_batch_given_d (:499-535) and
//! compute_membership_witnesses_for_batch (vb_accumulator/src/positive.rs:369-381), transcribed below line by line.
//!
//!   DOCK_GPU_LIB_DIR=<repo>/crypto_amd cargo test --release --test parity_accumulator_issue
use ark_bls12_381::{Fr, G1Affine, G1Projective};
use ark_ec::{AffineRepr, CurveGroup};
use ark_ff::{batch_inversion, One, Zero};
use ark_std::rand::{rngs::StdRng, SeedableRng};
use ark_std::UniformRand;
use dock_gpu::accumulator_issue::{d_for_batch, membership_witnesses, non_membership_witnesses, CannotBeZero, ResidentMembers};
use dock_gpu::*;

fn setup() { assert!(init(0, 1 << 16), "no MI355X / libdock_gpu.so"); }
fn frs(rng: &mut StdRng, n: usize) -> Vec<Fr> { (0..n).map(|_| Fr::rand(rng)).collect() }

// universal.rs:479-495
fn cpu_d_for_batch(non_members: &[Fr], members: &[Fr]) -> Vec<Fr> {
    let mut ds = vec![Fr::one(); non_members.len()];
    for member in members { for (i, e) in non_members.iter().enumerate() { ds[i] *= *member - *e; } }
    ds
}
// universal.rs:509-526 and positive.rs:375-380: the scalars, then the same group element times each of them
fn cpu_points(base: &G1Affine, numerators: &[Fr], ys: &[Fr], alpha: &Fr) -> Vec<G1Affine> {
    let mut inv: Vec<Fr> = ys.iter().map(|y| *y + *alpha).collect();
    batch_inversion(&mut inv);
    G1Projective::normalize_batch(&numerators.iter().zip(inv.iter()).map(|(n, d)| *base * (*n * *d)).collect::<Vec<_>>())
}

#[test]
fn d_for_batch_host_partitioned_and_resident() {
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED00D1);
    let (members, mut ys) = (frs(&mut rng, 1000), frs(&mut rng, 300));
    for (m, n) in [(1usize, 1usize), (3, 33), (255, 32), (256, 1000), (300, 1000), (5, 0)] {
        assert_eq!(d_for_batch(&ys[..m], &members[..n], None).expect("d"), cpu_d_for_batch(&ys[..m], &members[..n]), "m = {}, n = {}", m, n);
    }
    let whole = cpu_d_for_batch(&ys, &members);
    for cut in [0usize, 1, 500, 999, 1000] {                         // universal.rs:476-478: partition the members, multiply the outputs
        let d1 = d_for_batch(&ys, &members[..cut], None).expect("first part");
        assert_eq!(d_for_batch(&ys, &members[cut..], Some(&d1)).expect("second part"), whole);
    }
    let res = ResidentMembers::new(&members).expect("upload");
    assert_eq!(res.len(), 1000);
    for off in [0usize, 1, 7] {
        assert_eq!(res.d_for_batch(&ys, off, 1000 - off, None).expect("resident"), cpu_d_for_batch(&ys, &members[off..]));
    }
    let d1 = res.d_for_batch(&ys, 0, 400, None).expect("resident part");
    assert_eq!(res.d_for_batch(&ys, 400, 600, Some(&d1)).expect("resident part"), whole);
    assert!(res.d_for_batch(&ys, 1, 1000, None).is_none());           // past the end
    ys[7] = members[999];                                             // a "non-member" that is a member: d = 0
    let d = d_for_batch(&ys, &members, None).expect("d");
    assert!(d[7].is_zero() && d.iter().filter(|x| x.is_zero()).count() == 1);
}

#[test]
fn witnesses_equal_the_references_arithmetic() {
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED00D2);
    let (alpha, f_v, v) = (Fr::rand(&mut rng), Fr::rand(&mut rng), Fr::rand(&mut rng));
    let (members, ys) = (frs(&mut rng, 500), frs(&mut rng, 257));
    let params_gen = (G1Affine::generator() * Fr::rand(&mut rng)).into_affine();
    let acc = (G1Affine::generator() * v).into_affine();
    let d = d_for_batch(&ys, &members, None).expect("d");
    for m in [1usize, 64, 257] {
        let want = cpu_points(&params_gen, &d[..m].iter().map(|x| f_v - *x).collect::<Vec<_>>(), &ys[..m], &alpha);
        assert_eq!(non_membership_witnesses(&d[..m], &ys[..m], &f_v, &alpha, &params_gen).expect("call").expect("no zero d"), want);
        assert_eq!(membership_witnesses(&ys[..m], &alpha, &acc).expect("call"), cpu_points(&acc, &vec![Fr::one(); m], &ys[..m], &alpha));
    }
    // the defining relation of a non-membership witness: (y + alpha) C + d P = f_V P
    let c = non_membership_witnesses(&d[..8], &ys[..8], &f_v, &alpha, &params_gen).unwrap().unwrap();
    for i in 0..8 { assert_eq!((c[i] * (ys[i] + alpha) + params_gen * d[i]).into_affine(), (params_gen * f_v).into_affine()); }
    // a membership witness verifies: (y + alpha) C = V
    let w = membership_witnesses(&ys[..8], &alpha, &acc).unwrap();
    for i in 0..8 { assert_eq!((w[i] * (ys[i] + alpha)).into_affine(), acc); }
    let mut bad = d[..8].to_vec();
    bad[7] = Fr::zero();
    assert_eq!(non_membership_witnesses(&bad, &ys[..8], &f_v, &alpha, &params_gen).expect("call"), Err(CannotBeZero));      // universal.rs:506-508
    let mut minus = ys[..8].to_vec();
    minus[0] = -alpha;                                                // no inverse: refused, the caller stays on its own path
    assert!(membership_witnesses(&minus, &alpha, &acc).is_none() && non_membership_witnesses(&d[..8], &minus, &f_v, &alpha, &params_gen).is_none());
    assert!(membership_witnesses(&ys[..3], &alpha, &G1Affine::identity()).unwrap().iter().all(|p| p.is_zero()));
}
