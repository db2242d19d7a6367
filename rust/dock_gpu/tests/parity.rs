//! rust/dock_gpu/tests/parity.rs — the pin against REAL arkworks that the build image cannot run (no Rust toolchain there).
//!
//!   DOCK_GPU_LIB_DIR=<repo>/crypto_amd cargo test --release            (one MI355X visible)
//!
//! 1. the library == arkworks on seeded inputs: `msm_bigint` / `msm_unchecked` over G1 and G2 (edge cases included), the RAW Fp12 output of
//!    `multi_miller_loop`, `final_exponentiation` (arkworks' chain raises to 3 (p^12 - 1) / r: only same-chain code is comparable),
//!    every coefficient of `G2Prepared::from`, the verifier's mixed call;
//! 2. `write_golden` stores what ARKWORKS computed under <repo>/tests/golden/ark/*.json (schema: tests/golden/ark/README.md).  Those files
//!    are then checked everywhere without Rust: `tests/test_ark_golden.py` compares the CPU oracle with them (pinning the oracle: parity
//!    "partial" -> "green") and, on a GPU box, the library through its C ABI.
use ark_bls12_381::{Bls12_381, Fr, G1Affine, G1Projective, G2Affine, G2Projective};
use ark_ec::pairing::Pairing;
use ark_ec::{AffineRepr, CurveGroup, VariableBaseMSM};
use ark_ff::{BigInt, PrimeField, UniformRand, Zero};
use ark_std::rand::{rngs::StdRng, SeedableRng};
use dock_gpu::*;
use std::fmt::Write as _;

fn setup() { assert!(init(0, 1 << 16), "no MI355X / libdock_gpu.so"); unsafe { dgpu_set_min_gpu_n(1); } }
fn g1s(rng: &mut StdRng, n: usize) -> Vec<G1Affine> { G1Projective::normalize_batch(&(0..n).map(|_| G1Projective::rand(rng)).collect::<Vec<_>>()) }
fn g2s(rng: &mut StdRng, n: usize) -> Vec<G2Affine> { G2Projective::normalize_batch(&(0..n).map(|_| G2Projective::rand(rng)).collect::<Vec<_>>()) }
fn frs(rng: &mut StdRng, n: usize) -> Vec<Fr> { (0..n).map(|_| Fr::rand(rng)).collect() }
fn big(s: &[Fr]) -> Vec<BigInt<4>> { s.iter().map(|x| x.into_bigint()).collect() }

#[test]
fn msm_equals_arkworks() {
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED0001);
    for &n in &[1usize, 2, 31, 32, 33, 255, 600, 1 << 12, (1 << 13) + 1, 1 << 16] {
        let (b1, b2, s) = (g1s(&mut rng, n), g2s(&mut rng, n.min(1 << 12)), frs(&mut rng, n));
        let sb = big(&s);
        assert_eq!(msm_bigint_g1(&b1, &sb).into_affine(), G1Projective::msm_bigint(&b1, &sb).into_affine(), "G1 n = {n}");
        assert_eq!(msm_unchecked_g1(&b1, &s).into_affine(), G1Projective::msm_unchecked(&b1, &s).into_affine());
        let m = b2.len();
        assert_eq!(msm_bigint_g2(&b2, &sb[..m]).into_affine(), G2Projective::msm_bigint(&b2, &sb[..m]).into_affine(), "G2 n = {m}");
        // the truncation the prover relies on (prover.rs:286): one scalar more than bases
        if n > 1 { assert_eq!(msm_bigint_g1(&b1[..n - 1], &sb).into_affine(), G1Projective::msm_bigint(&b1[..n - 1], &sb[..n - 1]).into_affine()); }
    }
    // edge cases: identity bases, zero / one / r - 1 scalars, P and -P, all-equal scalars
    let n = 300;
    let mut b = g1s(&mut rng, n);
    let mut s = frs(&mut rng, n);
    b[3] = G1Affine::identity(); b[7] = (-b[6].into_group()).into_affine();
    s[0] = Fr::zero(); s[1] = Fr::from(1u64); s[2] = -Fr::from(1u64); s[7] = s[6];
    assert_eq!(msm_unchecked_g1(&b, &s).into_affine(), G1Projective::msm_unchecked(&b, &s).into_affine());
    let same = vec![s[9]; n];
    assert_eq!(msm_unchecked_g1(&b, &same).into_affine(), G1Projective::msm_unchecked(&b, &same).into_affine());
    let r1 = ResidentG1::upload(&b, None);
    assert_eq!(r1.msm_bigint(1, &big(&s[1..])).into_affine(), G1Projective::msm_bigint(&b[1..], &big(&s[1..])).into_affine());
}

#[test]
fn pairing_equals_arkworks() {
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED0002);
    for &n in &[1usize, 2, 3, 4, 5, 64, 130, 1024] {
        let (mut p, mut q) = (g1s(&mut rng, n), g2s(&mut rng, n));
        if n >= 5 { p[1] = G1Affine::identity(); q[4] = G2Affine::identity(); }
        let f = multi_miller_loop(&p, &q);
        let g = Bls12_381::multi_miller_loop(p.iter().copied(), q.iter().copied());
        assert_eq!(f.0, g.0, "raw Miller output, n = {n}");
        assert_eq!(final_exponentiation(f).unwrap().0, Bls12_381::final_exponentiation(g).unwrap().0);
        assert_eq!(multi_pairing(&p, &q), Bls12_381::multi_pairing(p.iter().copied(), q.iter().copied()));
        let batch = final_exponentiation_batch(&[f, ark_ec::pairing::MillerLoopOutput(<Bls12_381 as Pairing>::TargetField::zero()), f]).unwrap();
        let want = Bls12_381::final_exponentiation(g);
        assert_eq!((batch[0], batch[1], batch[2]), (want, None, want), "final_exponentiation_batch, n = {n}");
    }
    let q = g2s(&mut rng, 7);
    let (mine, theirs): (Vec<G2Prepared>, Vec<G2Prepared>) = (g2_prepare(&q), q.iter().map(|x| G2Prepared::from(*x)).collect());
    for (a, b) in mine.iter().zip(theirs.iter()) { assert_eq!(a.infinity, b.infinity); assert_eq!(a.ell_coeffs, b.ell_coeffs); }
    // the verifier's call shape (verifier.rs:69-76): one affine pair, two prepared
    let p = g1s(&mut rng, 3);
    let f = multi_miller_loop_mixed(&p[..1], &q[..1], &p[1..], &theirs[1..3]);
    let g = Bls12_381::multi_miller_loop(p.iter().copied(), theirs[..3].iter().cloned());
    assert_eq!(f.0, g.0);
}

// ---- golden files: ARKWORKS' results, consumed by tests/test_ark_golden.py ---------------------------------------------------------------
fn hexw(w: &[u64]) -> String { let mut s = String::with_capacity(w.len() * 16); for x in w { write!(s, "{:016x}", x).unwrap(); } s }
fn norm_g1(p: G1Projective) -> Vec<u64> { // the ABI's normalised Jacobian: (x, y, 1) or (1, 1, 0)
    let a = p.into_affine();
    let one = ark_bls12_381::Fq::from(1u64);
    let mut w = Vec::new();
    if a.is_zero() { w.extend_from_slice(&one.0 .0); w.extend_from_slice(&one.0 .0); w.extend_from_slice(&[0u64; 6]); }
    else { w.extend_from_slice(&a.x.0 .0); w.extend_from_slice(&a.y.0 .0); w.extend_from_slice(&one.0 .0); }
    w
}
fn norm_g2(p: G2Projective) -> Vec<u64> {
    let a = p.into_affine();
    let one = ark_bls12_381::Fq::from(1u64);
    let mut w = Vec::new();
    let one2 = |w: &mut Vec<u64>| { w.extend_from_slice(&one.0 .0); w.extend_from_slice(&[0u64; 6]); };
    if a.is_zero() { one2(&mut w); one2(&mut w); w.extend_from_slice(&[0u64; 12]); }
    else { for c in [&a.x.c0, &a.x.c1, &a.y.c0, &a.y.c1] { w.extend_from_slice(&c.0 .0); } one2(&mut w); }
    w
}
fn scal_words(s: &[BigInt<4>]) -> Vec<u64> { s.iter().flat_map(|b| b.0).collect() }

#[test]
#[ignore = "writes tests/golden/ark/*.json: run with `cargo test --release -- --ignored write_golden`"]
fn write_golden() {
    let mut rng = StdRng::seed_from_u64(0x5EED00A2);
    let dir = concat!(env!("CARGO_MANIFEST_DIR"), "/../../tests/golden/ark");
    std::fs::create_dir_all(dir).unwrap();
    let head = "\"schema\": \"dock_gpu/ark-golden/1\", \"producer\": \"ark-ec ^0.4.1 / ark-ff ^0.4.1 / ark-bls12-381 ^0.4.0 (rust/dock_gpu/tests/parity.rs write_golden)\"";
    // MSM
    let mut cases = Vec::new();
    for &n in &[1usize, 2, 33, 300, 1025] {
        let (b1, s) = (g1s(&mut rng, n), big(&frs(&mut rng, n)));
        let (xy, inf) = pack_g1(&b1);
        cases.push(format!("{{\"kind\": \"msm_g1\", \"n\": {n}, \"bases\": \"{}\", \"inf\": \"{}\", \"scalars\": \"{}\", \"out\": \"{}\"}}",
                           hexw(&xy), inf.iter().map(|b| b.to_string()).collect::<String>(), hexw(&scal_words(&s)), hexw(&norm_g1(G1Projective::msm_bigint(&b1, &s)))));
        let m = n.min(300);
        let b2 = g2s(&mut rng, m);
        let (xy2, inf2) = pack_g2(&b2);
        cases.push(format!("{{\"kind\": \"msm_g2\", \"n\": {m}, \"bases\": \"{}\", \"inf\": \"{}\", \"scalars\": \"{}\", \"out\": \"{}\"}}",
                           hexw(&xy2), inf2.iter().map(|b| b.to_string()).collect::<String>(), hexw(&scal_words(&s[..m])), hexw(&norm_g2(G2Projective::msm_bigint(&b2, &s[..m])))));
    }
    std::fs::write(format!("{dir}/msm.json"), format!("{{{head}, \"cases\": [\n{}\n]}}\n", cases.join(",\n"))).unwrap();
    // pairings
    let mut cases = Vec::new();
    for &n in &[1usize, 2, 3, 4, 5, 9, 64] {
        let (p, q) = (g1s(&mut rng, n), g2s(&mut rng, n));
        let f = Bls12_381::multi_miller_loop(p.iter().copied(), q.iter().copied());
        let e = Bls12_381::final_exponentiation(f).unwrap();
        cases.push(format!("{{\"kind\": \"miller_loop\", \"n\": {n}, \"p\": \"{}\", \"q\": \"{}\", \"out\": \"{}\", \"final_exponentiation\": \"{}\"}}",
                           hexw(&pack_g1(&p).0), hexw(&pack_g2(&q).0), hexw(&fq12_to_words(&f.0)), hexw(&fq12_to_words(&e.0))));
    }
    let q = g2s(&mut rng, 2);
    for x in q.iter() {
        let pre = G2Prepared::from(*x);
        let mut w = Vec::new();
        for (c0, c1, c2) in pre.ell_coeffs.iter() { for c in [c0, c1, c2] { w.extend_from_slice(&c.c0 .0 .0); w.extend_from_slice(&c.c1 .0 .0); } }
        cases.push(format!("{{\"kind\": \"g2_prepared\", \"q\": \"{}\", \"coeffs\": \"{}\"}}", hexw(&pack_g2(&[*x]).0), hexw(&w)));
    }
    std::fs::write(format!("{dir}/pairing.json"), format!("{{{head}, \"cases\": [\n{}\n]}}\n", cases.join(",\n"))).unwrap();
}

// ---- the generic drop-ins (src/generic.rs): what rust/patches routes the reference's generic call sites to ----------------------------------
/// a function that is generic the way the reference's call sites are (utils/src/pairs.rs:143-147): it cannot name G1Affine
fn pairs_msm<G: AffineRepr>(left: &[G], right: &[G::ScalarField]) -> G::Group { dock_gpu::generic::msm_unchecked(left, right) }
fn coeff<G: AffineRepr>(query: &[G], assignment: &[<G::ScalarField as PrimeField>::BigInt]) -> G::Group { dock_gpu::generic::msm_bigint::<G>(&query[1..], assignment) }
fn checker_verify<E: Pairing>(a: Vec<E::G1Prepared>, b: Vec<E::G2Prepared>) -> Option<ark_ec::pairing::PairingOutput<E>> {
    dock_gpu::generic::final_exponentiation::<E>(dock_gpu::generic::multi_miller_loop::<E>(a, b))
}

#[test]
fn generic_wrappers_dispatch_and_fall_through() {
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED0007);
    for &n in &[3usize, 64, 600, 1 << 13] {
        let (b1, b2, s) = (g1s(&mut rng, n), g2s(&mut rng, n.min(1 << 11)), frs(&mut rng, n));
        let sb = big(&s);
        // BLS12-381: served by the library, equal to arkworks
        assert_eq!(pairs_msm::<G1Affine>(&b1, &s).into_affine(), G1Projective::msm_unchecked(&b1, &s).into_affine());
        assert_eq!(pairs_msm::<G2Affine>(&b2, &s[..b2.len()]).into_affine(), G2Projective::msm_unchecked(&b2, &s[..b2.len()]).into_affine());
        assert_eq!(coeff::<G1Affine>(&b1, &sb).into_affine(), G1Projective::msm_bigint(&b1[1..], &sb).into_affine());
        assert_eq!(dock_gpu::generic::msm::<G1Affine>(&b1, &s[..n - 1]), Err(n - 1));
        let m = n.min(1 << 10);
        let pa: Vec<<Bls12_381 as Pairing>::G1Prepared> = b1[..m].iter().map(|p| (*p).into()).collect();
        let pb: Vec<<Bls12_381 as Pairing>::G2Prepared> = b2[..m.min(b2.len())].iter().map(|q| (*q).into()).collect();
        let pa = pa[..pb.len()].to_vec();
        assert_eq!(checker_verify::<Bls12_381>(pa.clone(), pb.clone()), Bls12_381::final_exponentiation(Bls12_381::multi_miller_loop(pa, pb)));
        assert_eq!(dock_gpu::generic::multi_pairing::<Bls12_381>(&b1[..pb_len(&b2, m)], &b2[..pb_len(&b2, m)]), Bls12_381::multi_pairing(&b1[..pb_len(&b2, m)], &b2[..pb_len(&b2, m)]));
        let g = dock_gpu::generic::scale_batch_g1::<Bls12_381>(&b1, sb[0], true);
        for (p, q) in b1.iter().zip(g.iter()) { assert_eq!((-p.mul_bigint(sb[0])).into_affine(), *q); }
    }
}
fn pb_len(b2: &[G2Affine], m: usize) -> usize { m.min(b2.len()) }

/// another curve goes straight through to arkworks: the same generic code path with a type the library does not serve
#[cfg(feature = "other-curve-test")]
#[test]
fn generic_wrappers_leave_other_curves_alone() {
    use ark_bn254::{Fr as BnFr, G1Affine as BnG1, G1Projective as BnG1P};
    let mut rng = StdRng::seed_from_u64(0x5EED0008);
    let b: Vec<BnG1> = BnG1P::normalize_batch(&(0..600).map(|_| BnG1P::rand(&mut rng)).collect::<Vec<_>>());
    let s: Vec<BnFr> = (0..600).map(|_| BnFr::rand(&mut rng)).collect();
    assert_eq!(pairs_msm::<BnG1>(&b, &s), BnG1P::msm_unchecked(&b, &s));
}

// ---- round 6: the resident-bases cache, the host-side wrappers (src/host.rs), the whole-call entry points ---------------------------------------------
use dock_gpu::host::{self, cache, HSource, HostProvingKey, R1cs, ShardedG1, ShardedG2, WindowTableG1, WindowTableG2};

/// the same `&[G1Affine]` twice, then again: the second call makes it resident, later calls hit; a refilled buffer is noticed, an announced edit too
#[test]
fn resident_bases_cache_same_slice_twice_and_mutated_slice() {
    setup();
    cache::clear(); assert!(cache::set_min_n(1 << 12));
    let mut rng = StdRng::seed_from_u64(0x5EED0009);
    let n = 40_000usize;
    let mut b = g1s(&mut rng, n);
    let s0 = cache::stats();
    for k in 0..4 {
        let s = big(&frs(&mut rng, n));
        assert_eq!(msm_bigint_g1(&b, &s).into_affine(), G1Projective::msm_bigint(&b, &s).into_affine(), "call {k}");
        assert_eq!(msm_bigint_g1(&b[1..], &s).into_affine(), G1Projective::msm_bigint(&b[1..], &s[..n - 1]).into_affine(), "&query[1..], call {k}");
    }
    let s1 = cache::stats();
    assert!(s1.fills > s0.fills && s1.hits >= s0.hits + 5, "{:?} -> {:?}", s0, s1);
    // another key in the same buffer: the answer must be the new key's, at once
    let other = g1s(&mut rng, n);
    b.copy_from_slice(&other);
    let s = big(&frs(&mut rng, n));
    assert_eq!(msm_bigint_g1(&b, &s).into_affine(), G1Projective::msm_bigint(&other, &s).into_affine());
    assert!(cache::stats().stale > s1.stale);
    // an in-place edit of one record, announced (or caught by the exact mode)
    for _ in 0..3 { let _ = msm_bigint_g1(&b, &s); }
    b[n / 2] = b[7];
    assert!(cache::invalidate(&b));
    assert_eq!(msm_bigint_g1(&b, &s).into_affine(), G1Projective::msm_bigint(&b, &s).into_affine());
    assert!(cache::verify_every_record());
    for _ in 0..3 { let _ = msm_bigint_g1(&b, &s); }
    b[n / 3] = b[9];
    assert_eq!(msm_bigint_g1(&b, &s).into_affine(), G1Projective::msm_bigint(&b, &s).into_affine());
    assert!(cache::verify_every_record() && cache::set_min_n(1 << 16));       // (the library's defaults)
    assert!(!host::error_string(DGPU_E_BADARG).is_empty() && host::device_count() >= 1 && host::context_count() >= 1 && host::set_device(0));
    // G2 and the Montgomery forms through the same entry points
    let (b2, sf) = (g2s(&mut rng, 5000), frs(&mut rng, 5000));
    assert_eq!(msm_unchecked_g2(&b2, &sf).into_affine(), G2Projective::msm_unchecked(&b2, &sf).into_affine());
    let r2 = ResidentG2::upload(&b2, None);
    assert_eq!(r2.msm_bigint(1, &big(&sf[1..])).into_affine(), G2Projective::msm_bigint(&b2[1..], &big(&sf[1..])).into_affine());
}

#[test]
fn sharded_msm_window_tables_and_serde() {
    // two contexts on the one GPU of a test box: every code path of the multi-GPU form except a second physical device
    assert!(host::init_devices(&[0, 0], 1 << 16), "no MI355X / libdock_gpu.so");
    unsafe { dgpu_set_min_gpu_n(1); }
    let mut rng = StdRng::seed_from_u64(0x5EED000A);
    let n = 20_000usize;
    let (b, b2, s) = (g1s(&mut rng, n), g2s(&mut rng, 3000), big(&frs(&mut rng, n)));
    let want = G1Projective::msm_bigint(&b, &s).into_affine();
    assert_eq!(msm_bigint_g1_sharded(&b, &s, 0).into_affine(), want);
    // the unmodified one-shot call sharding itself over the two contexts (each caches its chunk at the second sighting)
    assert!(host::set_auto_shard_min_n(1 << 12) && cache::set_min_n(1 << 12));
    for _ in 0..3 { assert_eq!(msm_bigint_g1(&b, &s).into_affine(), want); }
    assert!(host::set_auto_shard_min_n(0) && cache::set_min_n(1 << 16));
    let sh = ShardedG1::upload(&b, 0, true).expect("sharded upload");
    assert_eq!(sh.shards(), 2);
    assert_eq!(sh.msm_bigint(&s).into_affine(), want);
    let rs = sh.upload_scalars(&s).expect("sharded scalars");
    assert_eq!(sh.msm_resident(&rs).expect("resident").into_affine(), want);
    let sh2 = ShardedG2::upload(&b2, 0, false).expect("sharded upload G2");
    assert_eq!(sh2.msm_bigint(&s).into_affine(), G2Projective::msm_bigint(&b2, &s[..3000]).into_affine());
    // the multi-process form's fold (what follows the all-gather of the ranks' partial points)
    let parts = [G1Projective::msm_bigint(&b[..n / 2], &s[..n / 2]), G1Projective::msm_bigint(&b[n / 2..], &s[n / 2..]), G1Projective::zero()];
    assert_eq!(fold_g1(&parts).into_affine(), want);
    // fixed base: WindowTable / multiply_field_elems_with_same_group_elem (utils/src/msm.rs:8-62)
    let f = frs(&mut rng, 1000);
    let (g1, g2) = (b[0], b2[0]);
    let t1 = WindowTableG1::new(&g1).expect("table");
    let prod = t1.multiply_many(&f).expect("products");
    for (x, p) in f.iter().zip(prod.iter()) { assert_eq!((g1 * x).into_affine(), *p); }
    assert_eq!(fixed_base_g1(&g1, &f).unwrap(), prod);
    let hb = t1.multiply_many_to_bases(&f).expect("products as a bases handle");
    let mut out = [0u64; 18];
    assert_eq!(unsafe { dgpu_msm_g1_handle(hb, 0, s.as_ptr() as *const u64, 1000, 0, out.as_mut_ptr()) }, DGPU_OK);
    unsafe { dgpu_bases_free(hb); }
    let t2 = WindowTableG2::new(&g2).expect("table G2");
    let prod2 = t2.multiply_many(&f[..100]).expect("products G2");
    for (x, p) in f.iter().zip(prod2.iter()) { assert_eq!((g2 * x).into_affine(), *p); }
    assert_eq!(fixed_base_g2(&g2, &f[..100]).unwrap(), prod2);
    assert_eq!(dock_gpu::generic::fixed_base_msm::<G1Projective>(&g1, &f).unwrap().iter().map(|p| p.into_affine()).collect::<Vec<_>>(), prod);
    // canonical (de)serialisation == ark-serialize
    use ark_serialize::CanonicalSerialize;
    for compressed in [true, false] {
        let mut want_bytes = Vec::new();
        for p in b[..50].iter() { if compressed { p.serialize_compressed(&mut want_bytes).unwrap() } else { p.serialize_uncompressed(&mut want_bytes).unwrap() } }
        let got = serialize_g1(&b[..50], compressed).unwrap();
        assert_eq!(got, want_bytes);
        assert_eq!(deserialize_g1(&got, 50, compressed, true).unwrap(), b[..50].to_vec());
        let mut want2 = Vec::new();
        for p in b2[..20].iter() { if compressed { p.serialize_compressed(&mut want2).unwrap() } else { p.serialize_uncompressed(&mut want2).unwrap() } }
        let got2 = serialize_g2(&b2[..20], compressed).unwrap();
        assert_eq!(got2, want2);
        assert_eq!(deserialize_g2(&got2, 20, compressed, true).unwrap(), b2[..20].to_vec());
    }
}

// Witness::compute_update_using_secret_key_after_batch_updates' arithmetic (vb_accumulator/src/witness.rs:238-285, batch_utils.rs:102-106,171-199,328-359,448-454) with arkworks
fn cpu_accumulator_factors(additions: &[Fr], removals: &[Fr], alpha: &Fr, y: &Fr) -> (Fr, Fr) {
    use ark_ff::{Field, One};
    let d = |u: &[Fr]| u.iter().fold(Fr::one(), |a, e| (*e - *y) * a);
    let (d_a, d_d_inv) = (d(additions), d(removals).inverse().unwrap_or(Fr::zero()));      // batch_inversion leaves a zero
    let mut v_a = Fr::zero();
    for s in 0..additions.len() {
        let factor = additions[..s].iter().fold(Fr::one(), |a, e| a * (*e + *alpha));
        v_a += additions[s + 1..].iter().fold(factor, |a, e| a * (*e - *y));
    }
    let mut v_d = Fr::zero();
    for s in 0..removals.len() {
        let factor = removals[..s + 1].iter().fold(Fr::one(), |a, e| a * (*e + *alpha)).inverse().unwrap();
        v_d += removals[..s].iter().fold(factor, |a, e| a * (*e - *y));
    }
    let phi = additions.iter().fold(Fr::one(), |a, e| a * (*e + *alpha));
    (d_a * d_d_inv, (v_a - v_d * phi) * d_d_inv)
}

#[test]
fn accumulator_witness_update_with_the_secret_key() {
    use ark_ff::Field;
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED00AC);
    let (alpha, v) = (Fr::rand(&mut rng), Fr::rand(&mut rng));
    let (additions, removals, mut elements) = (frs(&mut rng, 40), frs(&mut rng, 25), frs(&mut rng, 300));
    elements[3] = removals[1];                                        // a removed holder: d_factor = 0 and the identity
    elements[5] = additions[2];                                       // a holder whose element was just added: d_factor = 0
    let g = G1Affine::generator();
    let acc = (g * v).into_affine();
    let mut wits = G1Projective::normalize_batch(&elements.iter().map(|y| g * (v * (*y + alpha).inverse().unwrap())).collect::<Vec<_>>());
    wits[7] = G1Affine::identity();
    for (a, r) in [(&additions[..], &removals[..]), (&additions[..], &removals[..0]), (&additions[..0], &removals[..]), (&additions[..1], &removals[..1])] {
        let want: Vec<(Fr, Fr)> = elements.iter().map(|y| cpu_accumulator_factors(a, r, &alpha, y)).collect();
        let (f, gg) = host::accumulator_update_factors(a, r, &alpha, &elements).expect("factors");
        assert_eq!(f, want.iter().map(|x| x.0).collect::<Vec<_>>());
        assert_eq!(gg, want.iter().map(|x| x.1).collect::<Vec<_>>());
        let (d, new_wits) = host::accumulator_update_witnesses(a, r, &alpha, &elements, &wits, &acc).expect("witnesses");
        assert_eq!(d, f);
        for i in 0..elements.len() { assert_eq!(new_wits[i], (wits[i] * want[i].0 + acc * want[i].1).into_affine(), "holder {}", i); }
        if !r.is_empty() { assert!(d[3].is_zero() && new_wits[3].is_zero()); }
        // an ordinary holder's new witness verifies against the new accumulator: C' (y + alpha) = V'
        let v_new = a.iter().fold(v, |x, e| x * (*e + alpha)) * r.iter().fold(Fr::from(1u64), |x, e| x * (*e + alpha)).inverse().unwrap();
        assert_eq!((new_wits[0] * (elements[0] + alpha)).into_affine(), (g * v_new).into_affine());
    }
    assert!(host::accumulator_update_witnesses(&additions, &removals, &alpha, &elements[..2], &wits[..3], &acc).is_none());
    assert!(host::accumulator_update_factors(&[-alpha], &removals, &alpha, &elements).is_none());      // an addition equal to -alpha: refused
}

// Poly_v_AD::generate's coefficients with arkworks' own arithmetic, lowest degree first (vb_accumulator/src/batch_utils.rs:115-140,271-300,433-440)
fn cpu_v_ad_coefficients(additions: &[Fr], removals: &[Fr], alpha: &Fr) -> Vec<Fr> {
    use ark_ff::{Field, One};
    let mul_lin = |p: &[Fr], u: &Fr| { let mut q = ark_std::vec![Fr::zero(); p.len() + 1]; for (k, c) in p.iter().enumerate() { q[k] += *c * *u; q[k + 1] -= *c; } q };      // p (u - x)
    let (mut s, mut f) = (Vec::<Fr>::new(), Fr::one());
    for a in additions { s = if s.is_empty() { ark_std::vec![] } else { mul_lin(&s, a) }; if s.is_empty() { s.push(f); } else { s[0] += f; } f *= *a + *alpha; }
    let (mut d, mut p, mut g) = (ark_std::vec![Fr::zero(); removals.len()], ark_std::vec![Fr::one()], Fr::one());
    for r in removals { g *= (*r + *alpha).inverse().unwrap(); for (k, c) in p.iter().enumerate() { d[k] += *c * g; } p = mul_lin(&p, r); }
    let mut c = ark_std::vec![Fr::zero(); additions.len().max(removals.len())];
    for (k, x) in s.iter().enumerate() { c[k] += *x; }
    for (k, x) in d.iter().enumerate() { c[k] -= *x * f; }
    while c.last().map_or(false, |x| x.is_zero()) { c.pop(); }
    c
}

#[test]
fn accumulator_update_from_public_information() {
    use ark_ff::Field;
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED00AD);
    let (alpha, v) = (Fr::rand(&mut rng), Fr::rand(&mut rng));
    let (additions, removals, mut elements) = (frs(&mut rng, 40), frs(&mut rng, 25), frs(&mut rng, 300));
    elements[3] = removals[1];                                        // a removed holder: CannotBeZero for that holder alone
    let g = G1Affine::generator();
    let acc = (g * v).into_affine();
    let wits = G1Projective::normalize_batch(&elements.iter().map(|y| g * (v * (*y + alpha).inverse().unwrap())).collect::<Vec<_>>());
    for (a, r) in [(&additions[..], &removals[..]), (&additions[..], &removals[..0]), (&additions[..0], &removals[..]), (&additions[..1], &removals[..1])] {
        let omega = host::accumulator_omega(a, r, &alpha, &acc).expect("omega");
        let want = cpu_v_ad_coefficients(a, r, &alpha);
        assert_eq!(omega, G1Projective::normalize_batch(&want.iter().map(|c| acc * *c).collect::<Vec<_>>()));
        let got = host::accumulator_update_witnesses_public(a, r, &omega, &elements, &wits).expect("public update");
        let (d_sk, w_sk) = host::accumulator_update_witnesses(a, r, &alpha, &elements, &wits, &acc).expect("witnesses");
        let v_new = a.iter().fold(v, |x, e| x * (*e + alpha)) * r.iter().fold(Fr::from(1u64), |x, e| x * (*e + alpha)).inverse().unwrap();
        for i in 0..elements.len() {
            if r.contains(&elements[i]) { assert!(i == 3 && got[i].is_err()); continue; }      // removed in THIS pair's list only: elsewhere holder 3 is an ordinary holder
            let (d, w) = got[i].unwrap();
            assert_eq!((d, w), (d_sk[i], w_sk[i]), "holder {}", i);
            assert_eq!((w * (elements[i] + alpha)).into_affine(), (g * v_new).into_affine());
        }
    }
    let same = [additions[0]];
    assert!(host::accumulator_omega(&same, &same, &alpha, &acc).expect("omega").is_empty());      // 1 - (a + alpha) / (a + alpha): the zero polynomial
    assert!(host::accumulator_omega(&[-alpha], &removals, &alpha, &acc).is_none());
}

#[test]
fn many_small_msms_over_one_key() {
    // m rows against m arkworks calls: the shapes of dkgith.rs:174-192 (many short rows), one row of the key's full length, an identity row, &[Fr] and BigInt rows
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED0A11);
    let (b, b2) = (g1s(&mut rng, 600), g2s(&mut rng, 200));
    let (k1, k2) = (ResidentG1::upload(&b, None), ResidentG2::upload(&b2, None));
    for (m, n, off) in [(1usize, 1usize, 0usize), (300, 1, 5), (64, 24, 1), (17, 33, 0), (5, 600, 0), (3, 129, 7)] {
        let mut rows: Vec<Vec<Fr>> = (0..m).map(|_| frs(&mut rng, n)).collect();
        if m > 2 { for x in rows[m / 2].iter_mut() { *x = Fr::from(0u64); } }
        let big: Vec<Vec<BigInt<4>>> = rows.iter().map(|r| r.iter().map(|x| x.into_bigint()).collect()).collect();
        let (rf, rb): (Vec<&[Fr]>, Vec<&[BigInt<4>]>) = (rows.iter().map(|r| &r[..]).collect(), big.iter().map(|r| &r[..]).collect());
        let got = k1.msm_many_unchecked(off, &rf);
        let gotb = k1.msm_many(off, &rb);
        assert_eq!(got.len(), m);
        for j in 0..m {
            let want = G1Projective::msm_unchecked(&b[off..off + n], &rows[j]);
            assert_eq!(got[j].into_affine(), want.into_affine(), "G1 row {} of {} x {}", j, m, n);
            assert_eq!(gotb[j].into_affine(), want.into_affine());
            assert_eq!(k1.msm_bigint(off, &big[j]).into_affine(), want.into_affine());
        }
        if off + n <= 200 {
            let got2 = k2.msm_many_unchecked(off, &rf);
            let got2b = k2.msm_many(off, &rb);
            for j in 0..m {
                let want = G2Projective::msm_unchecked(&b2[off..off + n], &rows[j]);
                assert_eq!(got2[j].into_affine(), want.into_affine(), "G2 row {} of {} x {}", j, m, n);
                assert_eq!(got2b[j].into_affine(), want.into_affine());
            }
        }
        if off == 0 {
            let gen = dock_gpu::generic::msm_many::<G1Affine>(&b[..n], &rf);
            for j in 0..m { assert_eq!(gen[j].into_affine(), got[j].into_affine()); }
        }
    }
    // the raw entry point: row_stride > n, identity flags
    let (m, n, stride) = (9usize, 20usize, 23usize);
    let s: Vec<BigInt<4>> = frs(&mut rng, m * stride).iter().map(|x| x.into_bigint()).collect();
    let (mut out, mut inf) = (vec![0u64; m * 18], vec![7u8; m]);
    assert_eq!(unsafe { dgpu_msm_g1_handle_many(k1.handle(), 2, s.as_ptr() as *const u64, stride, n, m, 0, out.as_mut_ptr(), inf.as_mut_ptr()) }, DGPU_OK);
    for j in 0..m {
        assert_eq!(inf[j], 0);
        assert_eq!(k1.msm_bigint(2, &s[j * stride..j * stride + n]).into_affine(), G1Projective::msm_bigint(&b[2..2 + n], &s[j * stride..j * stride + n]).into_affine());
    }
    assert_eq!(unsafe { dgpu_msm_g2_handle_many(k2.handle(), 0, s.as_ptr() as *const u64, stride, n, 0, 0, core::ptr::null_mut(), core::ptr::null_mut()) }, DGPU_OK);
}

#[test]
fn scalings_and_the_scaled_miller_loop() {
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED000B);
    let (p, q) = (g1s(&mut rng, 130), g2s(&mut rng, 130));
    let m = frs(&mut rng, 130);
    let mb = big(&m);
    let scaled = g1_scale_batch(&p, &mb[0], false).expect("scalings");
    for (x, y) in p.iter().zip(scaled.iter()) { assert_eq!(x.mul_bigint(mb[0]).into_affine(), *y); }
    let want = Bls12_381::multi_miller_loop(p.iter().zip(m.iter()).map(|(x, k)| (*x * k).into_affine()), q.iter().copied());
    assert_eq!(multi_miller_loop_scaled(&p, &mb, &q).0, want.0);
    let want1 = Bls12_381::multi_miller_loop(p.iter().map(|x| (*x * m[0]).into_affine()), q.iter().copied());
    assert_eq!(multi_miller_loop_scaled(&p, &mb[..1], &q).0, want1.0);
}

// ---- LegoGroth16: witness map, prover, verifier ---------------------------------------------------------------------------------------------------------
/// the reference's witness map (legogroth16/src/r1cs_to_qap.rs:150-210) restated over ark-poly for the comparison
fn cpu_witness_map(a: &[Vec<(Fr, usize)>], b: &[Vec<(Fr, usize)>], c: &[Vec<(Fr, usize)>], num_inputs: usize, num_constraints: usize, z: &[Fr]) -> Vec<Fr> {
    use ark_ff::Field;
    use ark_poly::{EvaluationDomain, GeneralEvaluationDomain};
    let domain = GeneralEvaluationDomain::<Fr>::new(num_constraints + num_inputs).unwrap();
    let d = domain.size();
    let eval = |row: &Vec<(Fr, usize)>| row.iter().map(|(k, i)| *k * z[*i]).sum::<Fr>();
    let (mut va, mut vb, mut vc) = (vec![Fr::zero(); d], vec![Fr::zero(); d], vec![Fr::zero(); d]);
    for i in 0..num_constraints { va[i] = eval(&a[i]); vb[i] = eval(&b[i]); vc[i] = eval(&c[i]); }
    va[num_constraints..num_constraints + num_inputs].copy_from_slice(&z[..num_inputs]);
    let coset = domain.get_coset(Fr::GENERATOR).unwrap();
    for v in [&mut va, &mut vb, &mut vc] { domain.ifft_in_place(v); coset.fft_in_place(v); }
    let zinv = domain.evaluate_vanishing_polynomial(Fr::GENERATOR).inverse().unwrap();
    let mut ab: Vec<Fr> = va.iter().zip(vb.iter()).zip(vc.iter()).map(|((x, y), w)| (*x * y - w) * zinv).collect();
    coset.ifft_in_place(&mut ab);
    ab
}
/// x_i = x_{i-1}^2 + i: m constraints, one public input — (matrices a, b, c, full assignment, num_inputs)
#[allow(clippy::type_complexity)]
fn square_chain(m: usize) -> (Vec<Vec<(Fr, usize)>>, Vec<Vec<(Fr, usize)>>, Vec<Vec<(Fr, usize)>>, Vec<Fr>, usize) {
    let one = Fr::from(1u64);
    let mut z = vec![one, Fr::from(3u64)];                              // (1, x_0 public)
    let (mut a, mut b, mut c) = (Vec::new(), Vec::new(), Vec::new());
    for i in 0..m {
        let prev = z[1 + i];
        z.push(prev * prev + Fr::from(i as u64 + 1));
        a.push(vec![(one, 1 + i)]); b.push(vec![(one, 1 + i)]);
        c.push(vec![(one, 2 + i), (-Fr::from(i as u64 + 1), 0)]);       // x_{i-1}^2 = x_i - (i + 1)
    }
    (a, b, c, z, 2)
}
struct SyntheticKey { alpha_g1: G1Affine, beta_g1: G1Affine, delta_g1: G1Affine, eta_delta_inv_g1: G1Affine, eta_gamma_inv_g1: G1Affine, beta_g2: G2Affine, delta_g2: G2Affine,
                      gamma_abc_g1: Vec<G1Affine>, cw: usize, a_query: Vec<G1Affine>, b_g1_query: Vec<G1Affine>, b_g2_query: Vec<G2Affine>, h_query: Vec<G1Affine>, l_query: Vec<G1Affine> }
/// what create_proof_and_committed_witnesses_with_assignment computes (prover.rs:267-383), with arkworks on the CPU, for ANY key material
fn cpu_proof(k: &SyntheticKey, h: &[Fr], inst: &[Fr], wit: &[Fr], r: Fr, s: Fr, v: Fr) -> (G1Affine, G2Affine, G1Affine, G1Affine) {
    let assignment: Vec<BigInt<4>> = inst[1..].iter().chain(wit.iter()).map(|x| x.into_bigint()).collect();
    let aux: Vec<BigInt<4>> = wit[k.cw..].iter().map(|x| x.into_bigint()).collect();
    let hb: Vec<BigInt<4>> = h.iter().map(|x| x.into_bigint()).collect();
    let coeff1 = |init: G1Projective, q: &[G1Affine], vk: G1Affine| init + q[0] + G1Projective::msm_bigint(&q[1..], &assignment) + vk;
    let g_a = coeff1(k.delta_g1 * r, &k.a_query, k.alpha_g1);
    let g1_b = if r.is_zero() { G1Projective::zero() } else { coeff1(k.delta_g1 * s, &k.b_g1_query, k.beta_g1) };
    let g2_b = k.delta_g2 * s + k.b_g2_query[0] + G2Projective::msm_bigint(&k.b_g2_query[1..], &assignment) + k.beta_g2;
    let g_c = g_a * s + g1_b * r - k.delta_g1 * (r * s) + G1Projective::msm_bigint(&k.l_query, &aux) + G1Projective::msm_bigint(&k.h_query, &hb) - k.eta_delta_inv_g1 * v;
    let committed: Vec<BigInt<4>> = wit[..k.cw].iter().map(|x| x.into_bigint()).collect();
    let g_d = G1Projective::msm_bigint(&k.gamma_abc_g1[inst.len()..inst.len() + k.cw], &committed) + k.eta_gamma_inv_g1 * v;
    (g_a.into_affine(), g2_b.into_affine(), g_c.into_affine(), g_d.into_affine())
}

#[test]
fn witness_map_many_rows_of_a_small_circuit() {
    setup();
    // D = 512: a whole statement per block on the device; five assignments of the same circuit, each row against the CPU map
    let m = (1usize << 9) - 2;
    let (a, b, c, z, num_inputs) = square_chain(m);
    let want_h = cpu_witness_map(&a, &b, &c, num_inputs, m, &z);
    let rows: Vec<Fr> = (0..5).flat_map(|_| z.iter().copied()).collect();
    let circuit = R1cs::upload(&a, &b, &c, z.len(), num_inputs, m).expect("resident circuit");
    let got = circuit.witness_map_many(&rows).expect("witness_map_many");
    assert_eq!(got.len(), 5 * want_h.len());
    for row in got.chunks(want_h.len()) { assert_eq!(row, &want_h[..]); }
    assert_eq!(host::witness_map_many(&a, &b, &c, z.len(), num_inputs, m, &rows).unwrap(), got);
    assert_eq!(dock_gpu::generic::witness_map_many::<Fr>(&a, &b, &c, z.len(), num_inputs, m, &rows).unwrap(), got);
    assert_eq!(circuit.witness_map_many(&[]).unwrap().len(), 0);
}

#[test]
fn witness_map_and_the_prover_for_a_host_held_key() {
    setup();
    cache::clear(); assert!(cache::set_min_n(1 << 10));
    let mut rng = StdRng::seed_from_u64(0x5EED000C);
    let m = (1usize << 13) - 2;
    let (a, b, c, z, num_inputs) = square_chain(m);
    let want_h = cpu_witness_map(&a, &b, &c, num_inputs, m, &z);
    // the drop-in of witness_map_from_matrices (circuit resident by content hash), twice: the second call finds the circuit
    for _ in 0..2 { assert_eq!(host::witness_map_from_matrices(&a, &b, &c, num_inputs, m, &z).expect("witness map"), want_h); }
    assert_eq!(dock_gpu::generic::witness_map_from_matrices::<Fr>(&a, &b, &c, num_inputs, m, &z).unwrap(), want_h);
    let circuit = host::resident_circuit(&a, &b, &c, z.len(), num_inputs, m).expect("resident circuit");
    assert_eq!(circuit.witness_map(&z).unwrap(), want_h);
    assert_eq!(R1cs::upload(&a, &b, &c, z.len(), num_inputs, m).unwrap().witness_map(&z).unwrap(), want_h);
    // a synthetic key of the circuit's shape (the prover's equations hold for any key material)
    let nv = z.len();
    let cw = 2usize;
    let g = g1s(&mut rng, 6);
    let g2 = g2s(&mut rng, 2);
    let key = SyntheticKey { alpha_g1: g[0], beta_g1: g[1], delta_g1: g[2], eta_delta_inv_g1: g[3], eta_gamma_inv_g1: g[4], beta_g2: g2[0], delta_g2: g2[1],
                             gamma_abc_g1: g1s(&mut rng, num_inputs + cw), cw, a_query: g1s(&mut rng, nv), b_g1_query: g1s(&mut rng, nv), b_g2_query: g2s(&mut rng, nv),
                             h_query: g1s(&mut rng, want_h.len() - 1), l_query: g1s(&mut rng, nv - num_inputs - cw) };
    let (inst, wit) = (&z[..num_inputs], &z[num_inputs..]);
    let (r, s, v) = (Fr::rand(&mut rng), Fr::rand(&mut rng), Fr::rand(&mut rng));
    let want = cpu_proof(&key, &want_h, inst, wit, r, s, v);
    let hpk = HostProvingKey { alpha_g1: key.alpha_g1, beta_g1: key.beta_g1, delta_g1: key.delta_g1, eta_delta_inv_g1: key.eta_delta_inv_g1, eta_gamma_inv_g1: key.eta_gamma_inv_g1,
                               beta_g2: key.beta_g2, delta_g2: key.delta_g2, gamma_abc_g1: &key.gamma_abc_g1, commit_witness_count: cw,
                               a_query: &key.a_query, b_g1_query: &key.b_g1_query, b_g2_query: &key.b_g2_query, h_query: &key.h_query, l_query: &key.l_query };
    // first proof: views uploaded for the call; second: the cache makes them resident; third: warm — with h from the host and with the circuit resident
    for k in 0..3 {
        assert_eq!(create_proof_host(&hpk, HSource::Coefficients(&want_h), inst, wit, r, s, v).expect("prove_host"), want, "proof {k}, h from the host");
        assert_eq!(create_proof_host(&hpk, HSource::Circuit(&circuit), inst, wit, r, s, v).expect("prove_host"), want, "proof {k}, circuit resident");
    }
    assert!(cache::stats().fills >= 5);
    // r = 0 (no B in G1, prover.rs:330)
    assert_eq!(create_proof_host(&hpk, HSource::Coefficients(&want_h), inst, wit, Fr::zero(), s, v).unwrap(), cpu_proof(&key, &want_h, inst, wit, Fr::zero(), s, v));
    // the generic form the patched prover calls
    let gen = dock_gpu::generic::legogroth16_create_proof::<Bls12_381>(&key.alpha_g1, &key.beta_g1, &key.delta_g1, &key.eta_delta_inv_g1, &key.eta_gamma_inv_g1, &key.beta_g2, &key.delta_g2,
        &key.gamma_abc_g1, cw, &key.a_query, &key.b_g1_query, &key.b_g2_query, &key.h_query, &key.l_query, dock_gpu::generic::H::Matrices(&a, &b, &c, num_inputs, m), inst, wit, r, s, v);
    assert_eq!(gen.expect("generic prover"), want);
    // the opt-in form with explicit handles (GpuProvingKey) gives the same proof
    let gpk = GpuProvingKey::upload(key.alpha_g1, key.beta_g1, key.delta_g1, key.eta_delta_inv_g1, key.eta_gamma_inv_g1, key.beta_g2, key.delta_g2, &key.gamma_abc_g1, cw,
                                    &key.a_query, &key.b_g1_query, &key.b_g2_query, &key.h_query, &key.l_query).expect("key upload");
    assert_eq!(create_proof_gpu(&gpk, circuit.handle(), &z, num_inputs, r, s, v).expect("prove"), want);
    assert!(cache::set_min_n(1 << 16));
}

/// a tiny hash-chain transcript for the aggregation round trip (both sides use the same one; the reference's is merlin)
#[derive(Clone)]
struct TestTranscript(u64);
impl TranscriptBytes for TestTranscript {
    fn append_message_bytes(&mut self, label: &[u8], bytes: &[u8]) {
        for b in label.iter().chain(bytes.iter()) { self.0 = (self.0 ^ *b as u64).wrapping_mul(0x100000001b3).rotate_left(23); }
    }
    fn challenge_fr(&mut self, label: &[u8]) -> Fr {
        self.append_message_bytes(label, b"challenge");
        let mut w = [0u8; 32];
        for (i, c) in w.chunks_mut(8).enumerate() { c.copy_from_slice(&self.0.wrapping_add(i as u64).wrapping_mul(0x9E3779B97F4A7C15).to_le_bytes()); }
        Fr::from_le_bytes_mod_order(&w)
    }
}

#[test]
fn verifier_batch_verifier_and_aggregation() {
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED000D);
    use ark_ec::Group;
    // a Groth16 key with known discrete logs and n valid proofs of it: e(A, B) = e(alpha, beta) e(C, delta) e(S, gamma), S = gamma_abc[0] + x gamma_abc[1]
    let (g, h) = (G1Projective::generator(), G2Projective::generator());
    let (al, be, ga, de, k0, k1) = (Fr::rand(&mut rng), Fr::rand(&mut rng), Fr::rand(&mut rng), Fr::rand(&mut rng), Fr::rand(&mut rng), Fr::rand(&mut rng));
    let (alpha_g1, beta_g2, gamma_g2, delta_g2) = ((g * al).into_affine(), (h * be).into_affine(), (h * ga).into_affine(), (h * de).into_affine());
    let gamma_abc = vec![(g * k0).into_affine(), (g * k1).into_affine()];
    let n = 8usize;
    let mut proofs = Vec::new();
    let mut inputs = Vec::new();
    for _ in 0..n {
        let (a, b, x) = (Fr::rand(&mut rng), Fr::rand(&mut rng), Fr::rand(&mut rng));
        use ark_ff::Field;
        let cc = (a * b - al * be - (k0 + x * k1) * ga) * de.inverse().unwrap();
        proofs.push(((g * a).into_affine(), (h * b).into_affine(), (g * cc).into_affine(), G1Affine::identity()));
        inputs.push(vec![x]);
    }
    let alpha_beta = Bls12_381::pairing(alpha_g1, beta_g2).0;
    let neg = |q: G2Affine| G2Prepared::from((-q.into_group()).into_affine());
    let pvk = GpuPreparedVerifyingKey::new(&alpha_beta, &neg(delta_g2), &neg(gamma_g2), &gamma_abc);
    for (p, x) in proofs.iter().zip(inputs.iter()) { assert_eq!(verify_proof_gpu(&pvk, &p.0, &p.1, &p.2, &p.3, x), Some(true)); }
    assert_eq!(verify_proof_gpu(&pvk, &proofs[0].0, &proofs[0].1, &proofs[1].2, &proofs[0].3, &inputs[0]), Some(false));
    assert_eq!(verify_proofs_batch_gpu(&pvk, &proofs, &inputs, Fr::rand(&mut rng)), Some(true));
    let mut bad = proofs.clone(); bad[3].2 = bad[2].2;
    assert_eq!(verify_proofs_batch_gpu(&pvk, &bad, &inputs, Fr::rand(&mut rng)), Some(false));
    let mut each = ark_std::vec![true; n]; each[3] = false;
    assert_eq!(verify_proofs_each_gpu(&pvk, &bad, &inputs), Some(each));
    // SnarkPack: aggregate the n proofs under a fake SRS (known alpha, beta), verify the aggregate
    let (sa, sb) = (Fr::rand(&mut rng), Fr::rand(&mut rng));
    let pow = |base: Fr, k: usize| { let mut v = Vec::with_capacity(k); let mut c = Fr::from(1u64); for _ in 0..k { v.push(c); c *= base; } v };
    let g_alpha: Vec<G1Affine> = pow(sa, 2 * n).iter().map(|e| (g * e).into_affine()).collect();
    let g_beta: Vec<G1Affine> = pow(sb, 2 * n).iter().map(|e| (g * e).into_affine()).collect();
    let h_alpha: Vec<G2Affine> = pow(sa, n).iter().map(|e| (h * e).into_affine()).collect();
    let h_beta: Vec<G2Affine> = pow(sb, n).iter().map(|e| (h * e).into_affine()).collect();
    let srs = GpuProverSrs::new(n, &g_alpha, &g_beta, &h_alpha, &h_beta, &h_alpha, &h_beta, &g_alpha[n..], &g_beta[n..]).expect("srs");
    let (pa, pb, pc): (Vec<G1Affine>, Vec<G2Affine>, Vec<G1Affine>) = (proofs.iter().map(|p| p.0).collect(), proofs.iter().map(|p| p.1).collect(), proofs.iter().map(|p| p.2).collect());
    let mut tp = TestTranscript(1);
    let words = aggregate_proofs_gpu(&srs, &mut tp, &pa, &pb, &pc, None).expect("aggregate");
    let mut tv = TestTranscript(1);
    let ok = verify_aggregate_proof_gpu(&g.into_affine(), &h.into_affine(), &g_alpha[1], &g_beta[1], &h_alpha[1], &h_beta[1], n, &alpha_g1, &beta_g2, &gamma_g2, &delta_g2, &gamma_abc,
                                        &inputs, &words, 0, None, Fr::rand(&mut rng), &mut tv, true);
    assert_eq!(ok, Some(true));
    assert_eq!(tp.0, tv.0, "prover and verifier leave the transcript in the same state");
    let mut tampered = words.clone(); let last = tampered.len() - 1; tampered[last] ^= 1;
    let mut tv2 = TestTranscript(1);
    assert_ne!(verify_aggregate_proof_gpu(&g.into_affine(), &h.into_affine(), &g_alpha[1], &g_beta[1], &h_alpha[1], &h_beta[1], n, &alpha_g1, &beta_g2, &gamma_g2, &delta_g2, &gamma_abc,
                                          &inputs, &tampered, 0, None, Fr::rand(&mut rng), &mut tv2, true), Some(true));
}

#[test]
fn device_deserialization_and_validation() {
    setup();
    use ark_serialize::{CanonicalDeserialize, CanonicalSerialize, Valid};
    let mut rng = StdRng::seed_from_u64(0x5EED00DE);
    let (b1, b2) = (g1s(&mut rng, 300), g2s(&mut rng, 60));
    for compressed in [true, false] {
        let (mut e1, mut e2) = (Vec::new(), Vec::new());
        for p in b1.iter() { if compressed { p.serialize_compressed(&mut e1).unwrap() } else { p.serialize_uncompressed(&mut e1).unwrap() } }
        for p in b2.iter() { if compressed { p.serialize_compressed(&mut e2).unwrap() } else { p.serialize_uncompressed(&mut e2).unwrap() } }
        let want1: Vec<G1Affine> = e1.chunks(e1.len() / b1.len()).map(|c| if compressed { G1Affine::deserialize_compressed(c).unwrap() } else { G1Affine::deserialize_uncompressed(c).unwrap() }).collect();
        assert_eq!(deserialize_g1_device(&e1, b1.len(), compressed, true).unwrap(), want1);
        assert_eq!(deserialize_g1_device(&e1, b1.len(), compressed, false).unwrap(), want1);
        let want2: Vec<G2Affine> = e2.chunks(e2.len() / b2.len()).map(|c| if compressed { G2Affine::deserialize_compressed(c).unwrap() } else { G2Affine::deserialize_uncompressed(c).unwrap() }).collect();
        assert_eq!(deserialize_g2_device(&e2, b2.len(), compressed, true).unwrap(), want2);
        // resident bases from bytes == resident bases from the points
        let s: Vec<BigInt<4>> = frs(&mut rng, b1.len()).iter().map(|f| f.into_bigint()).collect();
        let r1 = ResidentG1::from_serialized(&e1, b1.len(), compressed, true).ok().unwrap();
        assert_eq!(r1.msm_bigint(0, &s), G1Projective::msm_bigint(&b1, &s));
        let r2 = ResidentG2::from_serialized(&e2, b2.len(), compressed, true).ok().unwrap();
        assert_eq!(r2.msm_bigint(0, &s[..b2.len()]), G2Projective::msm_bigint(&b2, &s[..b2.len()]));
    }
    // a point on the curve outside G1 (x = 0: order 3): refused with validation at its index, accepted without, as arkworks does
    let mut e = Vec::new();
    for p in b1[..5].iter() { p.serialize_compressed(&mut e).unwrap(); }
    let mut off = [0u8; 48]; off[0] = 0x80;                                 // x = 0, y = 2 (not the largest root)
    let unchecked = G1Affine::deserialize_compressed_unchecked(&off[..]).unwrap();
    assert!(unchecked.is_on_curve() && !unchecked.is_in_correct_subgroup_assuming_on_curve() && unchecked.check().is_err());
    e[96..144].copy_from_slice(&off);
    assert_eq!(deserialize_g1_device(&e, 5, true, true), Err(Some(2)));
    assert_eq!(ResidentG1::from_serialized(&e, 5, true, true).err(), Some(Some(2)));
    assert_eq!(deserialize_g1_device(&e, 5, true, false).unwrap()[2], unchecked);
    // Valid::check on points in memory
    let mut pts = b1[..4].to_vec(); pts.push(unchecked); pts.push(G1Affine::identity());
    let want: Vec<bool> = pts.iter().map(|p| p.check().is_ok()).collect();
    assert_eq!(validate_g1_batch(&pts).unwrap(), want);
    let q: Vec<G2Affine> = b2[..3].to_vec();
    assert_eq!(validate_g2_batch(&q).unwrap(), q.iter().map(|p| p.check().is_ok()).collect::<Vec<bool>>());
}

// ---- LegoGroth16 key generation on the device (generator.rs:245-442, r1cs_to_qap.rs:105-147,212-223) --------------------------------------------------
#[test]
fn instance_map_and_key_generation_on_a_resident_circuit() {
    use ark_ff::Field;
    use ark_poly::{EvaluationDomain, GeneralEvaluationDomain};
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED0010);
    let m = 300usize;
    let (a, b, c, z, num_inputs) = square_chain(m);
    let nv = z.len();
    let circuit = R1cs::upload(&a, &b, &c, nv, num_inputs, m).expect("upload");
    let t = Fr::rand(&mut rng);
    // instance_map_with_evaluation restated over ark-poly
    let dom = GeneralEvaluationDomain::<Fr>::new(m + num_inputs).unwrap();
    let u = dom.evaluate_all_lagrange_coefficients(t);
    let (mut wa, mut wb, mut wc) = (vec![Fr::zero(); nv], vec![Fr::zero(); nv], vec![Fr::zero(); nv]);
    for j in 0..num_inputs { wa[j] = u[m + j]; }
    for i in 0..m {
        for (co, k) in &a[i] { wa[*k] += u[i] * co; }
        for (co, k) in &b[i] { wb[*k] += u[i] * co; }
        for (co, k) in &c[i] { wc[*k] += u[i] * co; }
    }
    let zt = dom.evaluate_vanishing_polynomial(t);
    assert_eq!(circuit.instance_map(t).expect("instance map"), (wa.clone(), wb.clone(), wc.clone(), zt, dom.size()));
    // the key: spot-checked against the closed form, then a proof made with it satisfies the verifier's equation
    let (alpha, beta, gamma, delta, eta) = (Fr::rand(&mut rng), Fr::rand(&mut rng), Fr::rand(&mut rng), Fr::rand(&mut rng), Fr::rand(&mut rng));
    let (g1, g2) = (G1Affine::generator(), G2Affine::generator());
    let cw = 1usize;
    let (pk, vk) = generate_parameters_gpu(&circuit, cw, alpha, beta, gamma, delta, eta, t, g1, g2).expect("setup");
    assert_eq!(vk.alpha_g1, (g1 * alpha).into_affine());
    assert_eq!(vk.delta_g2, (g2 * delta).into_affine());
    assert_eq!(vk.eta_gamma_inv_g1, (g1 * (eta * gamma.inverse().unwrap())).into_affine());
    let mix = |j: usize| beta * wa[j] + alpha * wb[j] + wc[j];
    assert_eq!(vk.gamma_abc_g1[1], (g1 * (mix(1) * gamma.inverse().unwrap())).into_affine());
    assert!(generate_parameters_gpu(&circuit, nv, alpha, beta, gamma, delta, eta, t, g1, g2).is_none());      // InsufficientWitnessesForCommitment
    let (r, s, v) = (Fr::rand(&mut rng), Fr::rand(&mut rng), Fr::rand(&mut rng));
    let (pa, pb, pc, pd) = create_proof_gpu(&pk, circuit.handle(), &z, num_inputs, r, s, v).expect("prove");
    // verify_qap_proof (verifier.rs:62-84): e(A, B) = e(alpha, beta) e(D, gamma) e(C, delta), D = proof.d + sum x_j gamma_abc[j]
    let mut d = pd.into_group();
    for j in 0..num_inputs { d += vk.gamma_abc_g1[j] * z[j]; }
    let lhs = Bls12_381::pairing(pa, pb);
    let rhs = Bls12_381::multi_pairing([vk.alpha_g1, d.into_affine(), pc], [(g2 * beta).into_affine(), vk.gamma_g2, vk.delta_g2]);
    assert_eq!(lhs, rhs);
}

// GT on the device over many elements against arkworks: mul_bigint per element, the sum of such, Valid::check
#[test]
fn gt_powers_on_the_device() {
    use ark_ec::pairing::PairingOutput;
    use ark_serialize::Valid;
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED0C07);
    let n = 70usize;
    let mut bases: Vec<PairingOutput<Bls12_381>> = (0..n).map(|_| Bls12_381::pairing(g1s(&mut rng, 1)[0], g2s(&mut rng, 1)[0])).collect();
    bases[3] = PairingOutput(Bls12_381::multi_miller_loop(g1s(&mut rng, 1), g2s(&mut rng, 1)).0);      // not in GT
    bases[9] = PairingOutput(<Bls12_381 as Pairing>::TargetField::zero());
    let mut exps: Vec<BigInt<4>> = (0..n).map(|_| ark_bls12_381::Fr::rand(&mut rng).into_bigint()).collect();
    exps[1] = BigInt::<4>([u64::MAX; 4]);
    let want: Vec<PairingOutput<Bls12_381>> = bases.iter().zip(exps.iter()).map(|(b, e)| PairingOutput(b.0.pow(e.0))).collect();
    assert_eq!(dock_gpu::host::gt_pow_batch(&bases, &exps).unwrap(), want);
    let prod = want.iter().fold(<Bls12_381 as Pairing>::TargetField::from(1u64), |acc, w| acc * w.0);
    assert_eq!(dock_gpu::host::gt_multi_pow_device(&bases, &exps).unwrap().0, prod);
    let ok = dock_gpu::host::gt_in_subgroup_device(&bases).unwrap();
    for (i, b) in bases.iter().enumerate() { assert_eq!(ok[i], !b.0.is_zero() && b.check().is_ok(), "element {i}"); }
}

// BBS+ in bulk against the reference's own SignatureG1::new / verify (bbs_plus/src/signature.rs:138-296): the e, s the reference drew go back in, so the A must agree
#[cfg(feature = "bbs-plus")]
#[test]
fn bbs_plus_bulk_equals_the_reference() {
    use bbs_plus::prelude::{KeypairG2, SignatureG1, SignatureParamsG1};
    use dock_gpu::bbs_plus::{sign_many, verify_batch, verify_each, GpuSignatureParams};
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED0BB5);
    for &(l, n) in &[(1usize, 3usize), (5, 65), (30, 257)] {
        let params = SignatureParamsG1::<Bls12_381>::generate_using_rng(&mut rng, l as u32);
        let keypair = KeypairG2::<Bls12_381>::generate_using_rng(&mut rng, &params);
        let msgs: Vec<Vec<Fr>> = (0..n).map(|_| frs(&mut rng, l)).collect();
        let rows: Vec<&[Fr]> = msgs.iter().map(|m| m.as_slice()).collect();
        let sigs: Vec<SignatureG1<Bls12_381>> = msgs.iter().map(|m| SignatureG1::new(&mut rng, m, &keypair.secret_key, &params).unwrap()).collect();
        let (e, s): (Vec<Fr>, Vec<Fr>) = sigs.iter().map(|x| (x.e, x.s)).unzip();
        let gp = GpuSignatureParams::new(&params, &keypair.public_key).expect("parameters");
        assert_eq!(gp.supported_message_count(), l);
        let mine = sign_many(&gp, &keypair.secret_key, &rows, &e, &s).expect("sign_many");
        for i in 0..n { assert_eq!(mine[i].as_ref().expect("a signature"), &sigs[i], "l = {l}, row {i}"); }
        // a row the reference would draw e again for
        let mut e2 = e.clone(); e2[n - 1] = -keypair.secret_key.0;
        let flagged = sign_many(&gp, &keypair.secret_key, &rows, &e2, &s).expect("sign_many");
        assert!(flagged[n - 1].is_none() && flagged[..n - 1].iter().zip(sigs.iter()).all(|(a, b)| a.as_ref() == Some(b)));
        // verdicts: the reference's verify, signature by signature, on a batch with a wrong message, a wrong e and a swapped A
        let mut bad = sigs.clone();
        let mut bad_msgs = msgs.clone();
        bad_msgs[0][0] += Fr::from(1u64);
        if n > 2 { bad[1].e += Fr::from(1u64); let a = bad[n - 1].A; bad[n - 1].A = bad[n - 2].A; bad[n - 2].A = a; }
        let bad_rows: Vec<&[Fr]> = bad_msgs.iter().map(|m| m.as_slice()).collect();
        let want: Vec<bool> = bad.iter().zip(bad_msgs.iter()).map(|(x, m)| x.verify(m, keypair.public_key.clone(), params.clone()).is_ok()).collect();
        assert_eq!(verify_each(&gp, &bad, &bad_rows).expect("verify_each"), want);
        assert!(verify_each(&gp, &sigs, &rows).expect("verify_each").iter().all(|&k| k));
        let rho = Fr::rand(&mut rng);
        assert_eq!(verify_batch(&gp, &sigs, &rows, &rho), Some(true));
        assert_eq!(verify_batch(&gp, &bad, &bad_rows, &rho), Some(false));
    }
}

// BBS+ proofs of knowledge in bulk against the reference's own PoKOfSignatureG1Proof::verify (bbs_plus/src/proof.rs:355-611): the same Ok / first error, proof by proof
#[cfg(feature = "bbs-plus")]
#[test]
fn bbs_plus_pok_bulk_equals_the_reference() {
    use bbs_plus::prelude::{KeypairG2, MessageOrBlinding, PoKOfSignatureG1Proof, PoKOfSignatureG1Protocol, SignatureG1, SignatureParamsG1};
    use dock_gpu::bbs_plus::{pok_verify_batch, pok_verify_each, GpuSignatureParams};
    use std::collections::{BTreeMap, BTreeSet};
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED0B0C);
    for &(l, n) in &[(1usize, 3usize), (5, 65), (30, 257)] {
        let params = SignatureParamsG1::<Bls12_381>::generate_using_rng(&mut rng, l as u32);
        let keypair = KeypairG2::<Bls12_381>::generate_using_rng(&mut rng, &params);
        let gp = GpuSignatureParams::new(&params, &keypair.public_key).expect("parameters");
        let (mut proofs, mut revealed, mut challenges): (Vec<PoKOfSignatureG1Proof<Bls12_381>>, Vec<BTreeMap<usize, Fr>>, Vec<Fr>) = (vec![], vec![], vec![]);
        for i in 0..n {
            let msgs = frs(&mut rng, l);
            let sig = SignatureG1::new(&mut rng, &msgs, &keypair.secret_key, &params).unwrap();
            // every proof its own pattern: nothing revealed, everything, every (i % 5 + 2)-th message
            let ids: BTreeSet<usize> = match i % 3 { 0 => BTreeSet::new(), 1 => (0..l).collect(), _ => (0..l).filter(|j| j % (i % 5 + 2) == 0).collect() };
            let protocol = PoKOfSignatureG1Protocol::init(&mut rng, &sig, &params,
                msgs.iter().enumerate().map(|(j, m)| if ids.contains(&j) { MessageOrBlinding::RevealMessage(m) } else { MessageOrBlinding::BlindMessageRandomly(m) })).unwrap();
            let c = Fr::rand(&mut rng);
            proofs.push(protocol.gen_proof(&c).unwrap());
            revealed.push(ids.iter().map(|&j| (j, msgs[j])).collect());
            challenges.push(c);
        }
        let maps: Vec<&BTreeMap<usize, Fr>> = revealed.iter().collect();
        let all = pok_verify_each(&gp, &proofs, &maps, &challenges, None).expect("pok_verify_each");
        assert!(all.iter().all(|r| r.is_ok()), "l = {l}");
        let rho = Fr::rand(&mut rng);
        assert_eq!(pok_verify_batch(&gp, &proofs, &maps, &challenges, None, &rho), Some(true));
        // one tamper of every kind the reference tells apart, and the reference's verdict beside ours
        let mut bad = proofs.clone();
        let mut bad_c = challenges.clone();
        bad[0].sc_resp_1.response1 += Fr::from(1u64);
        if n > 4 {
            bad[1].T2 = bad[2].T2;
            bad[2].A_prime = G1Affine::zero();
            let (a, b) = (bad[3].A_prime, bad[3].A_bar);
            bad[3].A_bar = (b + a).into_affine();
            bad_c[4] += Fr::from(1u64);
        }
        let mine = pok_verify_each(&gp, &bad, &maps, &bad_c, None).expect("pok_verify_each");
        for i in 0..n {
            let theirs = bad[i].verify(&revealed[i], &bad_c[i], keypair.public_key.clone(), params.clone());
            assert_eq!(format!("{:?}", mine[i]), format!("{:?}", theirs), "l = {l}, proof {i}");
        }
        assert!(mine[0].is_err());
        assert_eq!(pok_verify_batch(&gp, &bad, &maps, &bad_c, None, &rho), Some(false));
    }
}

// the 2023 scheme in bulk against the reference's own Signature23G1::new / verify (bbs_plus/src/signature_23.rs) and both PoKOfSignature23G1Proof::verify
// (proof_23_cdl.rs:302-549, proof_23_ietf.rs:244-479): the same A, the same Ok / first error, proof by proof; one verdict for the batch
#[cfg(feature = "bbs-plus")]
#[test]
fn bbs23_bulk_equals_the_reference() {
    use bbs_plus::prelude::{KeypairG2, MessageOrBlinding};
    use bbs_plus::proof_23_cdl::{PoKOfSignature23G1Proof as CdlProof, PoKOfSignature23G1Protocol as CdlProtocol};
    use bbs_plus::proof_23_ietf::{PoKOfSignature23G1Proof as IetfProof, PoKOfSignature23G1Protocol as IetfProtocol};
    use bbs_plus::setup::SignatureParams23G1;
    use bbs_plus::signature_23::Signature23G1;
    use dock_gpu::bbs_plus::{pok_ietf_verify_batch_23, pok_ietf_verify_each_23, pok_verify_batch_23, pok_verify_each_23, sign_many_23, verify_batch_23, verify_each_23,
                             GpuSignatureParams23};
    use std::collections::{BTreeMap, BTreeSet};
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED2023);
    for &(l, n) in &[(1usize, 3usize), (5, 65), (30, 257)] {
        let params = SignatureParams23G1::<Bls12_381>::generate_using_rng(&mut rng, l as u32);
        let keypair = KeypairG2::<Bls12_381>::generate_using_rng_and_bbs23_params(&mut rng, &params);
        let msgs: Vec<Vec<Fr>> = (0..n).map(|_| frs(&mut rng, l)).collect();
        let rows: Vec<&[Fr]> = msgs.iter().map(|m| m.as_slice()).collect();
        let sigs: Vec<Signature23G1<Bls12_381>> = msgs.iter().map(|m| Signature23G1::new(&mut rng, m, &keypair.secret_key, &params).unwrap()).collect();
        let e: Vec<Fr> = sigs.iter().map(|x| x.e).collect();
        let gp = GpuSignatureParams23::new(&params, &keypair.public_key).expect("parameters");
        assert_eq!(gp.supported_message_count(), l);
        let mine = sign_many_23(&gp, &keypair.secret_key, &rows, &e).expect("sign_many_23");
        for i in 0..n { assert_eq!(mine[i].as_ref().expect("a signature"), &sigs[i], "l = {l}, row {i}"); }
        let mut e2 = e.clone(); e2[n - 1] = -keypair.secret_key.0;
        let flagged = sign_many_23(&gp, &keypair.secret_key, &rows, &e2).expect("sign_many_23");
        assert!(flagged[n - 1].is_none() && flagged[..n - 1].iter().zip(sigs.iter()).all(|(a, b)| a.as_ref() == Some(b)));
        let mut bad = sigs.clone();
        let mut bad_msgs = msgs.clone();
        bad_msgs[0][0] += Fr::from(1u64);
        if n > 2 { bad[1].e += Fr::from(1u64); let a = bad[n - 1].A; bad[n - 1].A = bad[n - 2].A; bad[n - 2].A = a; }
        let bad_rows: Vec<&[Fr]> = bad_msgs.iter().map(|m| m.as_slice()).collect();
        let want: Vec<bool> = bad.iter().zip(bad_msgs.iter()).map(|(x, m)| x.verify(m, keypair.public_key.clone(), params.clone()).is_ok()).collect();
        assert_eq!(verify_each_23(&gp, &bad, &bad_rows).expect("verify_each_23"), want);
        assert!(verify_each_23(&gp, &sigs, &rows).expect("verify_each_23").iter().all(|&k| k));
        let rho = Fr::rand(&mut rng);
        assert_eq!(verify_batch_23(&gp, &sigs, &rows, &rho), Some(true));
        assert_eq!(verify_batch_23(&gp, &bad, &bad_rows, &rho), Some(false));

        // proofs of both kinds over the same signatures, every proof its own pattern: nothing revealed, everything, every (i % 5 + 2)-th message
        let (mut cdl, mut ietf, mut revealed, mut challenges): (Vec<CdlProof<Bls12_381>>, Vec<IetfProof<Bls12_381>>, Vec<BTreeMap<usize, Fr>>, Vec<Fr>) = (vec![], vec![], vec![], vec![]);
        for i in 0..n {
            let ids: BTreeSet<usize> = match i % 3 { 0 => BTreeSet::new(), 1 => (0..l).collect(), _ => (0..l).filter(|j| j % (i % 5 + 2) == 0).collect() };
            let mb = |m: &Vec<Fr>| -> Vec<MessageOrBlinding<Fr>> {
                m.iter().enumerate().map(|(j, v)| if ids.contains(&j) { MessageOrBlinding::RevealMessage(v) } else { MessageOrBlinding::BlindMessageRandomly(v) }).collect()
            };
            let c = Fr::rand(&mut rng);
            cdl.push(CdlProtocol::init(&mut rng, &sigs[i], &params, mb(&msgs[i])).unwrap().gen_proof(&c).unwrap());
            ietf.push(IetfProtocol::init(&mut rng, &sigs[i], &params, mb(&msgs[i])).unwrap().gen_proof(&c).unwrap());
            revealed.push(ids.iter().map(|&j| (j, msgs[i][j])).collect());
            challenges.push(c);
        }
        let maps: Vec<&BTreeMap<usize, Fr>> = revealed.iter().collect();
        assert!(pok_verify_each_23(&gp, &cdl, &maps, &challenges, None).expect("pok_verify_each_23").iter().all(|r| r.is_ok()), "l = {l}");
        assert!(pok_ietf_verify_each_23(&gp, &ietf, &maps, &challenges, None).expect("pok_ietf_verify_each_23").iter().all(|r| r.is_ok()), "l = {l}");
        assert_eq!(pok_verify_batch_23(&gp, &cdl, &maps, &challenges, None, &rho), Some(true));
        assert_eq!(pok_ietf_verify_batch_23(&gp, &ietf, &maps, &challenges, None, &rho), Some(true));
        // one tamper of every kind the reference tells apart, and the reference's verdict beside ours
        let (mut bad_cdl, mut bad_ietf, mut bad_c) = (cdl.clone(), ietf.clone(), challenges.clone());
        bad_cdl[0].sc_resp_1.response1 += Fr::from(1u64);
        bad_ietf[0].T = bad_ietf[1].T;
        if n > 4 {
            bad_cdl[1].T2 = bad_cdl[2].T2;
            bad_cdl[2].A_bar = G1Affine::zero();
            bad_ietf[2].A_bar = G1Affine::zero();
            let (a, b) = (bad_cdl[3].A_bar, bad_cdl[3].B_bar);
            bad_cdl[3].B_bar = (b + a).into_affine();
            bad_c[4] += Fr::from(1u64);
        }
        let mine = pok_verify_each_23(&gp, &bad_cdl, &maps, &bad_c, None).expect("pok_verify_each_23");
        let mine_ietf = pok_ietf_verify_each_23(&gp, &bad_ietf, &maps, &bad_c, None).expect("pok_ietf_verify_each_23");
        for i in 0..n {
            let theirs = bad_cdl[i].verify(&revealed[i], &bad_c[i], keypair.public_key.clone(), params.clone());
            assert_eq!(format!("{:?}", mine[i]), format!("{:?}", theirs), "CDL, l = {l}, proof {i}");
            let theirs = bad_ietf[i].verify(&revealed[i], &bad_c[i], keypair.public_key.clone(), params.clone());
            assert_eq!(format!("{:?}", mine_ietf[i]), format!("{:?}", theirs), "IETF, l = {l}, proof {i}");
        }
        assert!(mine[0].is_err() && mine_ietf[0].is_err());
        assert_eq!(pok_verify_batch_23(&gp, &bad_cdl, &maps, &bad_c, None, &rho), Some(false));
        assert_eq!(pok_ietf_verify_batch_23(&gp, &bad_ietf, &maps, &bad_c, None, &rho), Some(false));
    }
}

// accumulator proofs in bulk against the reference's own MembershipProof::verify and NonMembershipProof::verify (vb_accumulator/src/proofs_cdh.rs:138-149, :365-387):
// the same Ok / first error, proof by proof; one verdict for the batch
#[cfg(feature = "vb-accumulator")]
#[test]
fn accumulator_proofs_bulk_equal_the_reference() {
    use ark_ff::Field;
    use dock_gpu::accumulator_proofs::{membership_verify_batch, membership_verify_each, non_membership_verify_batch, non_membership_verify_each, GpuAccumulatorVerifier};
    use vb_accumulator::proofs_cdh::{MembershipProof, MembershipProofProtocol, NonMembershipProof, NonMembershipProofProtocol};
    use vb_accumulator::setup::{Keypair, SetupParams};
    use vb_accumulator::witness::{MembershipWitness, NonMembershipWitness};
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED0ACC);
    let params = SetupParams::<Bls12_381>::generate_using_rng(&mut rng);
    let keypair = Keypair::<Bls12_381>::generate_using_rng(&mut rng, &params);
    let alpha = keypair.secret_key.0;
    let key = GpuAccumulatorVerifier::new(&params, &keypair.public_key).expect("key");
    let v = (params.P * Fr::rand(&mut rng)).into_affine();
    let q = G1Affine::rand(&mut rng);
    for &n in &[3usize, 65, 257] {
        // membership: C = 1 / (y + alpha) V
        let (mut proofs, mut challenges): (Vec<MembershipProof<Bls12_381>>, Vec<Fr>) = (vec![], vec![]);
        for _ in 0..n {
            let y = Fr::rand(&mut rng);
            let wit = MembershipWitness((v * (y + alpha).inverse().unwrap()).into_affine());
            let c = Fr::rand(&mut rng);
            proofs.push(MembershipProofProtocol::<Bls12_381>::init(&mut rng, y, None, &v, &wit).gen_proof(&c).unwrap());
            challenges.push(c);
        }
        let rho = Fr::rand(&mut rng);
        assert!(membership_verify_each(&key, &v, &proofs, &challenges, None).expect("membership_verify_each").iter().all(|r| r.is_ok()), "n = {n}");
        assert_eq!(membership_verify_batch(&key, &v, &proofs, &challenges, None, &rho), Some(true));
        let (mut bad, mut bad_c) = (proofs.clone(), challenges.clone());
        bad[0].0.sc.as_mut().unwrap().response1 += Fr::from(1u64);
        bad[1].0.A_prime = G1Affine::zero();
        let (a, b) = (bad[2].0.A_prime, bad[2].0.A_bar);
        bad[2].0.A_bar = (b + a).into_affine();
        if n > 3 { bad_c[3] += Fr::from(1u64); }
        let mine = membership_verify_each(&key, &v, &bad, &bad_c, None).expect("membership_verify_each");
        for i in 0..n {
            let theirs = bad[i].verify(&v, &bad_c[i], keypair.public_key.clone(), params.clone());
            assert_eq!(format!("{:?}", mine[i]), format!("{:?}", theirs), "n = {n}, membership proof {i}");
        }
        assert!(mine[0].is_err());
        assert_eq!(membership_verify_batch(&key, &v, &bad, &bad_c, None, &rho), Some(false));

        // non-membership: C (y + alpha) + d P = V
        let (mut proofs, mut challenges): (Vec<NonMembershipProof<Bls12_381>>, Vec<Fr>) = (vec![], vec![]);
        for _ in 0..n {
            let (y, d) = (Fr::rand(&mut rng), Fr::rand(&mut rng));
            let wit = NonMembershipWitness { d, C: ((v.into_group() - params.P * d) * (y + alpha).inverse().unwrap()).into_affine() };
            let c = Fr::rand(&mut rng);
            proofs.push(NonMembershipProofProtocol::<Bls12_381>::init(&mut rng, y, None, v, &wit, &params, q).gen_proof(&c).unwrap());
            challenges.push(c);
        }
        assert!(non_membership_verify_each(&key, &v, &q, &proofs, &challenges, None).expect("non_membership_verify_each").iter().all(|r| r.is_ok()), "n = {n}");
        assert_eq!(non_membership_verify_batch(&key, &v, &q, &proofs, &challenges, None, &rho), Some(true));
        let (mut bad, mut bad_c) = (proofs.clone(), challenges.clone());
        bad[0].sc_2.response += Fr::from(1u64);
        bad[1].J = G1Affine::zero();
        bad[2].t_1 = bad[0].t_1;
        if n > 3 {
            bad[3].C_prime = G1Affine::zero();
            let (a, b) = (bad[4].C_prime, bad[4].C_bar);
            bad[4].C_bar = (b + a).into_affine();
            bad_c[5] += Fr::from(1u64);
        }
        let mine = non_membership_verify_each(&key, &v, &q, &bad, &bad_c, None).expect("non_membership_verify_each");
        for i in 0..n {
            let theirs = bad[i].verify(v, &bad_c[i], keypair.public_key.clone(), params.clone(), q);
            assert_eq!(format!("{:?}", mine[i]), format!("{:?}", theirs), "n = {n}, non-membership proof {i}");
        }
        assert!(mine[0].is_err());
        assert_eq!(non_membership_verify_batch(&key, &v, &q, &bad, &bad_c, None, &rho), Some(false));
    }
}

// the accumulator proofs with a GT commitment in bulk (src/accumulator_gt_proofs.rs) against the reference's own `MembershipProof::verify` /
// `NonMembershipProof::verify` of vb_accumulator/src/proofs.rs: the same error per proof, or one verdict.  NOT compiled in the build image.
#[cfg(all(feature = "vb-accumulator", not(any(feature = "saver", feature = "smc-range-proof", feature = "bulletproofs-plus-plus"))))]
#[test]
fn accumulator_gt_proofs_bulk_equal_the_reference() {
    use ark_ec::pairing::PairingOutput;
    use ark_ff::Field;
    use dock_gpu::accumulator_gt_proofs::{membership_verify_batch, membership_verify_each, non_membership_verify_batch, non_membership_verify_each, GpuAccumulatorGtVerifier};
    use vb_accumulator::proofs::{MembershipProof, MembershipProofProtocol, NonMembershipProof, NonMembershipProofProtocol};
    use vb_accumulator::setup::{Keypair, NonMembershipProvingKey, SetupParams};
    use vb_accumulator::witness::{MembershipWitness, NonMembershipWitness};
    setup();
    let mut rng = StdRng::seed_from_u64(0x5EED0AC6);
    let params = SetupParams::<Bls12_381>::generate_using_rng(&mut rng);
    let keypair = Keypair::<Bls12_381>::generate_using_rng(&mut rng, &params);
    let alpha = keypair.secret_key.0;
    let nm_prk = NonMembershipProvingKey::<G1Affine>::generate_using_rng(&mut rng);
    let prk = nm_prk.derive_membership_proving_key();
    let key = GpuAccumulatorGtVerifier::new(&params, &keypair.public_key).expect("key");
    let v = (params.P * Fr::rand(&mut rng)).into_affine();
    for &n in &[3usize, 65, 257] {
        // membership: C = 1 / (y + alpha) V
        let (mut proofs, mut challenges): (Vec<MembershipProof<Bls12_381>>, Vec<Fr>) = (vec![], vec![]);
        for _ in 0..n {
            let y = Fr::rand(&mut rng);
            let wit = MembershipWitness((v * (y + alpha).inverse().unwrap()).into_affine());
            let c = Fr::rand(&mut rng);
            proofs.push(MembershipProofProtocol::<Bls12_381>::init(&mut rng, y, None, &wit, &keypair.public_key, &params, &prk).gen_proof(&c).unwrap());
            challenges.push(c);
        }
        let rho = Fr::rand(&mut rng);
        assert!(membership_verify_each(&key, &v, &prk.0, &proofs, &challenges, None).expect("membership_verify_each").iter().all(|r| r.is_ok()), "n = {n}");
        assert_eq!(membership_verify_batch(&key, &v, &prk.0, &proofs, &challenges, None, &rho), Some(true));
        // every error of the reference's order, and a valid proof whose commitment is the identity is none
        let (mut bad, mut bad_c) = (proofs.clone(), challenges.clone());
        bad[0].schnorr_response.0.s_sigma += Fr::from(1u64);
        bad[1].schnorr_commit.0.R_rho = bad[0].schnorr_commit.0.R_rho;
        bad[2].schnorr_commit.0.R_E = PairingOutput(bad[2].schnorr_commit.0.R_E.0 * bad[0].schnorr_commit.0.R_E.0);
        if n > 3 {
            bad[3].schnorr_response.0.s_delta_sigma += Fr::from(1u64);
            bad[4].schnorr_commit.0.R_delta_rho = G1Affine::zero();
            bad[5].randomized_witness.0.E_C = bad[6].randomized_witness.0.E_C;
            bad_c[7] += Fr::from(1u64);
        }
        let mine = membership_verify_each(&key, &v, &prk.0, &bad, &bad_c, None).expect("membership_verify_each");
        for i in 0..n {
            let theirs = bad[i].verify(&v, &bad_c[i], keypair.public_key.clone(), params.clone(), &prk);
            assert_eq!(format!("{:?}", mine[i]), format!("{:?}", theirs), "n = {n}, membership proof {i}");
        }
        assert!(mine[0].is_err() && mine[2].is_err());
        assert_eq!(membership_verify_batch(&key, &v, &prk.0, &bad, &bad_c, None, &rho), Some(false));
        // a partial proof: the element's response travels beside it
        let y = Fr::rand(&mut rng);
        let wit = MembershipWitness((v * (y + alpha).inverse().unwrap()).into_affine());
        let (c, blinding) = (Fr::rand(&mut rng), Fr::rand(&mut rng));
        let partial = MembershipProofProtocol::<Bls12_381>::init(&mut rng, y, Some(blinding), &wit, &keypair.public_key, &params, &prk).gen_partial_proof(&c).unwrap();
        let resp = blinding + c * y;
        assert!(membership_verify_each(&key, &v, &prk.0, &[partial.clone()], &[c], Some(&[resp])).expect("partial")[0].is_ok());
        assert!(membership_verify_each(&key, &v, &prk.0, &[partial.clone()], &[c], Some(&[resp + Fr::from(1u64)])).expect("partial")[0].is_err());
        assert!(membership_verify_each(&key, &v, &prk.0, &[partial], &[c], None).is_none());      // MissingSchnorrResponseForElement stays with the caller

        // non-membership: C (y + alpha) + d P = V
        let (mut proofs, mut challenges): (Vec<NonMembershipProof<Bls12_381>>, Vec<Fr>) = (vec![], vec![]);
        for _ in 0..n {
            let (y, d) = (Fr::rand(&mut rng), Fr::rand(&mut rng));
            let wit = NonMembershipWitness { d, C: ((v.into_group() - params.P * d) * (y + alpha).inverse().unwrap()).into_affine() };
            let c = Fr::rand(&mut rng);
            proofs.push(NonMembershipProofProtocol::<Bls12_381>::init(&mut rng, y, None, &wit, &keypair.public_key, &params, &nm_prk).gen_proof(&c).unwrap());
            challenges.push(c);
        }
        assert!(non_membership_verify_each(&key, &v, &nm_prk, &proofs, &challenges, None).expect("non_membership_verify_each").iter().all(|r| r.is_ok()), "n = {n}");
        assert_eq!(non_membership_verify_batch(&key, &v, &nm_prk, &proofs, &challenges, None, &rho), Some(true));
        let (mut bad, mut bad_c) = (proofs.clone(), challenges.clone());
        bad[0].schnorr_response.s_v += Fr::from(1u64);
        bad[1].schnorr_commit.R_B = bad[0].schnorr_commit.R_B;
        bad[2].schnorr_commit.C.R_E = PairingOutput(bad[2].schnorr_commit.C.R_E.0 * bad[0].schnorr_commit.C.R_E.0);
        if n > 3 {
            bad[3].schnorr_response.C.s_rho += Fr::from(1u64);
            bad[4].randomized_witness.E_d_inv = G1Affine::zero();
            bad[5].schnorr_commit.C.R_delta_sigma = bad[6].schnorr_commit.C.R_delta_sigma;
            bad_c[7] += Fr::from(1u64);
        }
        let mine = non_membership_verify_each(&key, &v, &nm_prk, &bad, &bad_c, None).expect("non_membership_verify_each");
        for i in 0..n {
            let theirs = bad[i].verify(&v, &bad_c[i], keypair.public_key.clone(), params.clone(), &nm_prk);
            assert_eq!(format!("{:?}", mine[i]), format!("{:?}", theirs), "n = {n}, non-membership proof {i}");
        }
        assert!(mine[0].is_err() && mine[2].is_err());
        assert_eq!(non_membership_verify_batch(&key, &v, &nm_prk, &bad, &bad_c, None, &rho), Some(false));
    }
}

// PS (Coconut) signatures in bulk behind the reference's own types (src/coconut.rs) against the reference's `Signature::new` / `verify` and `SignaturePoK::verify`
#[cfg(feature = "coconut")]
#[test]
fn ps_bulk_equals_the_reference() {
    use ark_serialize::CanonicalSerialize;
    use coconut_crypto::setup::{PublicKey, SecretKey, SignatureParams};
    use coconut_crypto::{CommitMessage, Signature, SignaturePoK, SignaturePoKGenerator};
    use dock_gpu::coconut::{pok_verify_each, sign_many, verify_batch, verify_each, GpuPsParams};
    use std::collections::BTreeMap;
    setup();
    let mut rng = StdRng::seed_from_u64(0xC0C0);
    let bytes_of = |s: &Signature<Bls12_381>| { let mut b = vec![]; s.serialize_compressed(&mut b).unwrap(); b };
    for &(l, n) in &[(1usize, 3usize), (5, 65), (30, 257)] {
        let sk = SecretKey::<Fr>::rand(&mut rng, l as u32);
        let params = SignatureParams::<Bls12_381>::new::<blake2::Blake2b512>(b"dock_gpu parity", l as u32);
        let pk = PublicKey::new(&sk, &params);
        let msgs: Vec<Vec<Fr>> = (0..n).map(|_| frs(&mut rng, l)).collect();
        let rows: Vec<&[Fr]> = msgs.iter().map(|m| m.as_slice()).collect();
        let gp = GpuPsParams::new(&params, &pk).expect("parameters");
        assert_eq!(gp.supported_message_count(), l);
        // Signature::new draws r with Fr::rand as its only use of the generator: the same seed gives the reference the r handed to sign_many
        let r: Vec<Fr> = (0..n).map(|i| Fr::rand(&mut StdRng::seed_from_u64(1000 + i as u64))).collect();
        let sigs: Vec<Signature<Bls12_381>> = (0..n).map(|i| Signature::new(&mut StdRng::seed_from_u64(1000 + i as u64), &msgs[i], &sk, &params).unwrap()).collect();
        let mine = sign_many(&gp, &sk, &rows, &r).expect("sign_many");
        for i in 0..n { assert_eq!(bytes_of(&mine[i]), bytes_of(&sigs[i]), "l = {l}, row {i}"); }
        let mut r0 = r.clone(); r0[n - 1] = Fr::from(0u64);
        assert!(sign_many(&gp, &sk, &rows, &r0).expect("sign_many")[n - 1].is_zero());
        let mut bad = sigs.clone();
        let mut bad_msgs = msgs.clone();
        bad_msgs[0][0] += Fr::from(1u64);
        if n > 2 { bad.swap(n - 1, n - 2); }
        let bad_rows: Vec<&[Fr]> = bad_msgs.iter().map(|m| m.as_slice()).collect();
        let want: Vec<bool> = bad.iter().zip(bad_msgs.iter()).map(|(x, m)| x.verify(m, &pk, &params).is_ok()).collect();
        assert_eq!(verify_each(&gp, &bad, &bad_rows).expect("verify_each"), want);
        assert!(verify_each(&gp, &sigs, &rows).expect("verify_each").iter().all(|&k| k));
        let rho = Fr::rand(&mut rng);
        assert_eq!(verify_batch(&gp, &sigs, &rows, &rho), Some(true));
        assert_eq!(verify_batch(&gp, &bad, &bad_rows, &rho), Some(false));

        // proofs over the same signatures, every proof its own pattern: nothing revealed, everything, every (i % 5 + 2)-th message
        let (mut proofs, mut revealed, mut challenges): (Vec<SignaturePoK<Bls12_381>>, Vec<BTreeMap<usize, Fr>>, Vec<Fr>) = (vec![], vec![], vec![]);
        for i in 0..n {
            let shown = |j: usize| match i % 3 { 0 => false, 1 => true, _ => j % (i % 5 + 2) == 0 };
            let c = Fr::rand(&mut rng);
            let commit = msgs[i].iter().enumerate().map(|(j, m)| if shown(j) { CommitMessage::RevealMessage } else { CommitMessage::BlindMessageRandomly(*m) });
            proofs.push(SignaturePoKGenerator::init(&mut rng, commit, &sigs[i], &pk, &params).unwrap().gen_proof(&c).unwrap());
            revealed.push((0..l).filter(|&j| shown(j)).map(|j| (j, msgs[i][j])).collect());
            challenges.push(c);
        }
        let maps: Vec<&BTreeMap<usize, Fr>> = revealed.iter().collect();
        assert!(pok_verify_each(&gp, &proofs, &maps, &challenges).expect("pok_verify_each").iter().all(|r| r.is_ok()), "l = {l}");
        // a wrong challenge, a wrong revealed message, a proof checked against another row's messages: the reference's verdict beside ours
        let (mut bad_c, mut bad_rev) = (challenges.clone(), revealed.clone());
        bad_c[0] += Fr::from(1u64);
        if let Some(v) = bad_rev[1].values_mut().next() { *v += Fr::from(1u64); }
        let mut bad_proofs = proofs.clone();
        if n > 4 { bad_proofs.swap(3, 4); }
        let bad_maps: Vec<&BTreeMap<usize, Fr>> = bad_rev.iter().collect();
        let mine = pok_verify_each(&gp, &bad_proofs, &bad_maps, &bad_c);
        if let Some(mine) = mine {                                   // (None: a swapped proof's response count does not fit its row's mask — the reference errs there too)
            for i in 0..n {
                let theirs = bad_proofs[i].verify(&bad_c[i], bad_rev[i].iter().map(|(j, m)| (*j, m)), &pk, &params);
                assert_eq!(format!("{:?}", mine[i]), format!("{:?}", theirs), "l = {l}, proof {i}");
            }
            assert!(mine[0].is_err());
        }
    }
}

// SAVER in bulk behind the reference's own types (src/saver.rs) against the reference's decrypt_to_chunks_given_pairing_powers, verify_decryption,
// verify_ciphertext_commitment and verify_commitments_in_batch.  NOT compiled where it was written (no toolchain there).
#[cfg(feature = "saver")]
#[test]
fn saver_bulk_equals_the_reference() {
    use dock_gpu::saver::{decrypt_many, verify_commitment_each, verify_commitments_batch, verify_decryption_each, GpuCommitmentKey, GpuDecryptionKey};
    use saver::encryption::{Ciphertext, Encryption};
    use saver::keygen::{keygen, PreparedDecryptionKey};
    use saver::setup::EncryptionGens;
    use saver::utils::{chunks_count, decompose};
    setup();
    let mut rng = StdRng::seed_from_u64(0x5A7E);
    for &(b, n) in &[(4u8, 3usize), (8, 17)] {
        let k = chunks_count::<Fr>(b) as usize;
        let gens = EncryptionGens::<Bls12_381>::new_using_rng(&mut rng);
        let g_i: Vec<G1Affine> = (0..k).map(|_| G1Projective::rand(&mut rng).into_affine()).collect();
        let (delta_g, gamma_g) = (G1Projective::rand(&mut rng).into_affine(), G1Projective::rand(&mut rng).into_affine());
        let (sk, ek, dk) = keygen(&mut rng, b, &gens, &g_i, &delta_g, &gamma_g).unwrap();
        let gdk = GpuDecryptionKey::new(&dk, &g_i, &gens.H, b).expect("decryption key");
        assert_eq!(gdk.supported_chunks_count(), k);
        let powers = PreparedDecryptionKey::from(dk.clone()).pairing_powers(b, &g_i).unwrap();
        assert_eq!(gdk.pairing_powers().expect("powers"), powers);
        let msgs = frs(&mut rng, n);
        let mut cts: Vec<Ciphertext<Bls12_381>> = msgs.iter().map(|m| {
            let (c, _r) = Encryption::<Bls12_381>::encrypt_decomposed_message(&mut rng, decompose(m, b).unwrap(), &ek, &g_i).unwrap();
            Ciphertext { X_r: c[0], enc_chunks: c[1..k + 1].to_vec(), commitment: c[k + 1] }
        }).collect();
        cts[n - 1].enc_chunks[0] = g_i[0];                           // one ciphertext that does not decrypt, with a bad commitment
        let mine = decrypt_many(&gdk, &cts, &sk).expect("decrypt_many");
        let (mut all_chunks, mut all_nu) = (vec![], vec![]);
        for i in 0..n {
            let theirs = Encryption::<Bls12_381>::decrypt_to_chunks_given_pairing_powers(&cts[i].X_r, &cts[i].enc_chunks, &sk, dk.clone(), &g_i, b, Some(&powers));
            assert_eq!(format!("{:?}", mine[i]), format!("{:?}", theirs), "b = {b}, row {i}");
            let (c, nu) = mine[i].clone().unwrap_or((vec![0u16; k], G1Affine::identity()));
            all_chunks.push(c); all_nu.push(nu);
        }
        assert!(mine[n - 1].is_err());
        let rows: Vec<&[u16]> = all_chunks.iter().map(|c| c.as_slice()).collect();
        let ok = verify_decryption_each(&gdk, &cts, &rows, &all_nu).expect("verify_decryption_each");
        for i in 0..n {
            let theirs = Encryption::<Bls12_381>::verify_decryption(&all_chunks[i], &cts[i].X_r, &cts[i].enc_chunks, &all_nu[i], dk.clone(), &g_i, gens.clone());
            assert_eq!(ok[i], theirs.is_ok(), "row {i}");
        }
        let ck = GpuCommitmentKey::new(&ek, &gens.H).expect("commitment key");
        let each = verify_commitment_each(&ck, &cts).expect("verify_commitment_each");
        for i in 0..n { assert_eq!(each[i], cts[i].verify_commitment(ek.clone(), gens.clone()).is_ok(), "row {i}"); }
        assert!(!each[n - 1] && each[..n - 1].iter().all(|&v| v));
        let rho = Fr::rand(&mut rng);
        let r_powers: Vec<Fr> = (0..n).scan(Fr::from(1u64), |acc, _| { let v = *acc; *acc *= rho; Some(v) }).collect();
        assert_eq!(verify_commitments_batch(&ck, &cts, &r_powers), Some(false));
        assert_eq!(verify_commitments_batch(&ck, &cts[..n - 1], &r_powers[..n - 1]), Some(true));
        assert_eq!(Encryption::<Bls12_381>::verify_commitments_in_batch(&cts[..n - 1], &r_powers[..n - 1], ek.clone(), gens.clone()).is_ok(), true);
    }
}

// CLS / CCS range proofs over weak-BB signatures verified in bulk behind the reference's own types (src/smc_range_proof.rs) against the reference's own verify.
// NOT compiled where it was written (no toolchain there).
#[cfg(feature = "smc-range-proof")]
#[test]
fn smc_range_proofs_bulk_equal_the_reference() {
    use blake2::Blake2b512;
    use dock_gpu::smc_range_proof::{ccs_statement, ccs_verify_batch, ccs_verify_each, cls_statement, cls_verify_batch, cls_verify_each, GpuRangeVerifier};
    use smc_range_proof::ccs_set_membership::setup::{SetMembershipCheckParams, SetMembershipCheckParamsWithPairing};
    use smc_range_proof::common::MemberCommitmentKey;
    use smc_range_proof::prelude::{CCSArbitraryRangeProofProtocol, CLSRangeProofProtocol};
    setup();
    let mut rng = StdRng::seed_from_u64(0x5AC);
    for &(base, min, max) in &[(2u16, 0u64, u64::MAX), (3, 5, 13), (3, 5, 12), (4, 10, 11), (16, 0, 65536), (4, 10, 1000)] {
        let (params, _) = SetMembershipCheckParams::<Bls12_381>::new_for_range_proof::<_, Blake2b512>(&mut rng, b"test", base);
        let pp = SetMembershipCheckParamsWithPairing::from(params.clone());
        let comm_key = MemberCommitmentKey::<G1Affine>::generate_using_rng(&mut rng);
        let key = GpuRangeVerifier::new(&pp, &comm_key).expect("verifier");
        assert!(cls_statement(&key, max, min, base).is_err() && cls_statement(&key, min, max, base + 1).is_err());
        let n = 5usize;
        let values: Vec<u64> = (0..n as u64).map(|i| if i == 0 { min } else if i == 1 { max - 1 } else { min + (u64::rand(&mut rng) % (max - min)) }).collect();
        let (rs, cs) = (frs(&mut rng, n), frs(&mut rng, n));
        let comms: Vec<G1Affine> = values.iter().zip(&rs).map(|(v, r)| comm_key.commit(&Fr::from(*v), r)).collect();
        let random = frs(&mut rng, n);
        let rho = Fr::rand(&mut rng);

        let st = cls_statement(&key, min, max, base).unwrap();
        let mut proofs: Vec<_> = (0..n).map(|i| CLSRangeProofProtocol::init_given_base(&mut rng, values[i], rs[i], min, max, base, &comm_key, &params).unwrap().gen_proof(&cs[i])).collect();
        assert_eq!(cls_verify_batch(&key, &st, &comms, &proofs, &cs, &rho), Some(true));
        proofs[n - 1].D = comm_key.g;                                // InvalidRangeProof
        if let Some(p) = proofs[2].pok_sigs.last_mut() { p.A_bar = comm_key.h; }      // ShortGroupSig(InvalidProof)
        let mine = cls_verify_each(&key, &st, &comms, &proofs, &cs, None).expect("cls_verify_each");
        let merged = cls_verify_each(&key, &st, &comms, &proofs, &cs, Some(&random)).expect("cls_verify_each merged");
        for i in 0..n {
            let theirs = proofs[i].verify(&comms[i], &cs[i], min, max, &comm_key, pp.clone());
            assert_eq!(format!("{:?}", mine[i]), format!("{:?}", theirs), "cls base {base}, proof {i}");
            assert_eq!(merged[i].is_ok(), theirs.is_ok(), "cls merged base {base}, proof {i}");
        }
        assert!(mine[n - 1].is_err() && mine[0].is_ok());
        assert_eq!(cls_verify_batch(&key, &st, &comms, &proofs, &cs, &rho), Some(false));

        if max == u64::MAX || max == min + 1 { continue; }            // (base^l must fit the reference's u64; l = 0 is CLS's alone)
        let st = ccs_statement(&key, min, max, base).unwrap();
        let mut proofs: Vec<_> = (0..n).map(|i| CCSArbitraryRangeProofProtocol::init_given_base(&mut rng, values[i], rs[i], min, max, base, &comm_key, &params).unwrap().gen_proof(&cs[i])).collect();
        assert_eq!(ccs_verify_batch(&key, &st, &comms, &proofs, &cs, &rho).unwrap(), Some(true));
        proofs[n - 1].D_max = comm_key.g;
        proofs[2].pok_sigs_max[0].A_bar = comm_key.h;
        let mine = ccs_verify_each(&key, &st, &comms, &proofs, &cs, None).unwrap().expect("ccs_verify_each");
        for i in 0..n {
            let theirs = proofs[i].verify(&comms[i], &cs[i], min, max, &comm_key, pp.clone());
            assert_eq!(format!("{:?}", mine[i]), format!("{:?}", theirs), "ccs base {base}, proof {i}");
        }
        assert_eq!(ccs_verify_batch(&key, &st, &comms, &proofs, &cs, &rho).unwrap(), Some(false));
        proofs[1].pok_sigs_min.pop();
        assert!(ccs_verify_each(&key, &st, &comms, &proofs, &cs, None).is_err());      // ProofShorterThanExpected
    }
}

// Bulletproofs++ range proofs verified in bulk behind the reference's own types (src/bpp_range_proof.rs) against the reference's own verify.
// NOT compiled where it was written (no toolchain there).
#[cfg(feature = "bulletproofs-plus-plus")]
#[test]
fn bpp_range_proofs_bulk_equal_the_reference() {
    use blake2::Blake2b512;
    use bulletproofs_plus_plus::range_proof::Prover;
    use bulletproofs_plus_plus::setup::SetupParams;
    use dock_crypto_utils::transcript::new_merlin_transcript;
    use dock_gpu::bpp_range_proof::{challenges, verify_batch, verify_each, GpuSetup, Parts};
    setup();
    let mut rng = StdRng::seed_from_u64(0xB99);
    for &(base, num_bits, m) in &[(2u16, 8u16, 1usize), (2, 8, 2), (16, 8, 1), (4, 16, 4), (2, 64, 2)] {
        let sp = SetupParams::<G1Affine>::new_for_perfect_range_proof::<Blake2b512>(b"test", base, num_bits, m as u32);
        let gs = GpuSetup::new(&sp).expect("setup");
        let n = 5usize;
        let (mut vs, mut proofs) = (Vec::new(), Vec::new());
        for i in 0..n {
            let v: Vec<u64> = (0..m).map(|_| if i == 0 { 0 } else { u64::rand(&mut rng) >> (64 - num_bits) }).collect();
            let gamma = frs(&mut rng, m);
            let comms: Vec<G1Affine> = v.iter().zip(&gamma).map(|(v, g)| sp.compute_pedersen_commitment(*v, g)).collect();
            let mut t = new_merlin_transcript(b"BPP/tests");
            proofs.push(Prover::new_with_given_base(base, num_bits, comms.clone(), v, gamma).unwrap().prove(&mut rng, sp.clone(), &mut t).unwrap());
            vs.push(comms);
        }
        vs[n - 1][0] = sp.G;                                           // a commitment to another value
        let parts: Vec<Parts> = proofs.iter().map(|p| Parts::of(p).expect("parts")).collect();
        let chals: Vec<Vec<Fr>> = (0..n).map(|i| challenges(&mut new_merlin_transcript(b"BPP/tests"), num_bits, &vs[i], &parts[i])).collect();
        let mine = verify_each(&gs, num_bits, &vs, &parts, &chals).expect("verify_each");
        for i in 0..n {
            let theirs = proofs[i].verify(num_bits, &vs[i], &sp, &mut new_merlin_transcript(b"BPP/tests"));
            assert_eq!(mine[i].is_ok(), theirs.is_ok(), "base {base}, {num_bits} bits, {m} values, proof {i}");
        }
        assert!(mine[0].is_ok() && mine[n - 1] == Err(1));
        let rho = Fr::rand(&mut rng);
        assert_eq!(verify_batch(&gs, num_bits, &vs[..n - 1], &parts[..n - 1], &chals[..n - 1], &rho), Some(true));
        assert_eq!(verify_batch(&gs, num_bits, &vs, &parts, &chals, &rho), Some(false));
    }
}
