// rust/dock_gpu/build.rs — links libdock_gpu.so.  Same role as the reference's oblivious_transfer/build.rs:11-15 (the only FFI precedent in
// docknetwork/crypto: a `cc` build of c/transpose.c linked with #[link(name = "transpose")], src/util.rs:216-220); here the native code is a
// prebuilt shared library (hipcc is not something a cargo build should drive), found through DOCK_GPU_LIB_DIR.
fn main() {
    println!("cargo:rerun-if-env-changed=DOCK_GPU_LIB_DIR");
    let dir = std::env::var("DOCK_GPU_LIB_DIR").unwrap_or_else(|_| {
        // default: the in-tree build of this repository (crypto_amd/libdock_gpu.so, made by `python -c 'import __graft_entry__ as g; g.build()'`)
        let here = std::env::var("CARGO_MANIFEST_DIR").unwrap();
        format!("{}/../../crypto_amd", here)
    });
    println!("cargo:rustc-link-search=native={}", dir);
    // the feature `saver` (src/saver.rs, include/dock_gpu_saver.h) needs libdock_gpu_saver.so: the product's objects plus the SAVER calls, linked INSTEAD of it
    // the feature `smc-range-proof` (src/smc_range_proof.rs, include/dock_gpu_smc.h) needs libdock_gpu_smc.so in the same way; the two libraries are separate
    // images, so a host builds with one of the two features
    let name = if std::env::var("CARGO_FEATURE_SAVER").is_ok() { "dock_gpu_saver" } else if std::env::var("CARGO_FEATURE_SMC_RANGE_PROOF").is_ok() { "dock_gpu_smc" }
               else if std::env::var("CARGO_FEATURE_BULLETPROOFS_PLUS_PLUS").is_ok() { "dock_gpu_bpp" }      // (src/bpp_range_proof.rs, include/dock_gpu_bpp.h: libdock_gpu_bpp.so)
               // the feature `vb-accumulator` alone: libdock_gpu_acc_gt.so (src/accumulator_gt_proofs.rs, include/dock_gpu_acc_gt.h), which serves src/accumulator_proofs.rs as well
               else if std::env::var("CARGO_FEATURE_VB_ACCUMULATOR").is_ok() { "dock_gpu_acc_gt" } else { "dock_gpu" };
    println!("cargo:rustc-link-lib=dylib={}", name);
    println!("cargo:rustc-link-arg=-Wl,-rpath,{}", dir);
}
