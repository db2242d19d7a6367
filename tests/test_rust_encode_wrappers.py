"""CPU: the Rust wrappers of the device encoder and of the handle readers (public in rust/dock_gpu/src/encode.rs, their calls in src/host.rs) each have a
case in rust/dock_gpu/tests/encode_parity.rs, the crate exports the module, each public form forwards to a function host.rs defines, and every C entry
point those call is declared in ffi.rs with the arity passed (the build image has no Rust toolchain; tests/test_rust_shim_consistency.py does the
same for lib.rs and host.rs as a whole)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "rust", "dock_gpu")


def read(*p):
    return open(os.path.join(SRC, *p)).read()


def test_every_wrapper_has_a_parity_case_and_is_exported():
    enc, par, lib = read("src", "encode.rs"), read("tests", "encode_parity.rs"), read("src", "lib.rs")
    names = re.findall(r"pub fn (\w+)\s*\(", enc)
    assert sorted(names) == sorted(["serialize_g1_device", "serialize_g2_device", "bases_read_g1", "bases_read_g2", "bases_serialize_g1", "bases_serialize_g2"])
    for n in names:
        assert re.search(r"\b%s\(" % n, par), n
    assert "pub mod encode;" in lib and "pub use encode::*;" in lib


def test_ffi_calls_match_the_declarations():
    enc, host, ffi = read("src", "encode.rs"), read("src", "host.rs"), read("src", "ffi.rs")
    section = host[host.index("// ---- the encoding on the device, and resident bases read back"):]
    inner = re.findall(r"crate::host::(\w+)\(", enc)
    assert len(inner) == 6
    for name in inner:
        assert re.search(r"pub\(crate\) fn %s\(" % name, section), name
    decl = {m.group(1): len([a for a in m.group(2).split(",") if a.strip()]) for m in re.finditer(r"pub fn (dgpu_\w+)\(([^)]*)\)", ffi)}
    calls = re.findall(r"\b(dgpu_\w+)\(((?:[^()]|\([^()]*\))*)\)", section[:section.index("Some(out)\n}\n", section.index("fn handle_serialize_g2"))])
    assert sorted(c[0] for c in calls) == sorted("dgpu_%s" % f for f in ("g1_serialize_device", "g2_serialize_device", "bases_read_g1", "bases_read_g2", "bases_serialize_g1", "bases_serialize_g2"))
    for name, args in calls:
        depth, n = 0, 1
        for ch in args:
            depth += ch in "([{"
            depth -= ch in ")]}"
            n += ch == "," and depth == 0
        assert name in decl and decl[name] == n, (name, n, decl.get(name))
