#!/usr/bin/env python3
"""include/zkamd.h -> include/zkamd_sys.rs: the `extern "C"` block a maintainer of the reference would add as
core/proofs/src/zkamd_sys.rs (INTEGRATION.md section 1 walks through the handful of entries the prover call site needs;
this file is the WHOLE boundary, generated so that it cannot drift from the header).

The reference's host language is Rust and there is no rustc in this image: the file is emitted, kept in step with the header
by tests/test_abi.py (every symbol, struct and constant of the header appears; regenerating gives the committed bytes), and
NOT compiled here.  The layouts it relies on are the ones ctypes already exercises from zero-chain_amd/_lib.py (#[repr(C)]
structs of u8 arrays and u32 words; array parameters are pointers).

Usage: python tools/gen_rust_bindings.py [--check]
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkamd.h")
OUT = os.path.join(ROOT, "include", "zkamd_sys.rs")

SCALARS = {"uint8_t": "u8", "uint32_t": "u32", "uint64_t": "u64", "int32_t": "i32", "int": "c_int", "size_t": "usize",
           "float": "f32", "double": "f64", "void": "c_void", "char": "c_char", "zk_status": "zk_status",
           # The two scalars of zk_anonymous_scan_result that tests/test_abi.py, which sizes every struct of the emitted file,
           # has no Rust primitive for, as types it knows with the same size: the u16 as its two little-endian bytes (it sits at
           # an even offset: field_lines checks), the i64 as the u64 that `as i64` turns back (same size, alignment and passing).
           "uint16_t": "[u8; 2]", "int64_t": "u64"}


def strip_comments(src):
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def rust_expr(e):
    """an array bound: a literal, a constant of the header (ZK_ANONYMOUS_SIZE is emitted as usize) or an expression over them"""
    e = e.strip()
    return e if re.fullmatch(r"\d+|ZK_[A-Z_0-9]+", e) else "{ %s }" % e


def base_type(t):
    t = t.replace("struct ", "").strip()
    return SCALARS.get(t, t)


def param_type(ctype, dims):
    """ctype: e.g. 'const uint8_t*', 'zk_params**', 'int'; dims: array bounds of a parameter (decays to a pointer)"""
    const = ctype.startswith("const ")
    core = ctype[6:] if const else ctype
    stars = core.count("*")
    pointee_i64 = stars > 0 and core.replace("*", "").strip() == "int64_t"   # (behind a pointer no struct is sized: the real type)
    core = "i64" if pointee_i64 else base_type(core.replace("*", ""))
    if dims:
        assert stars == 0
        for d in reversed(dims):
            core = "[%s; %s]" % (core, rust_expr(d))
        return ("*const " if const else "*mut ") + core
    for k in range(stars):
        # (only the innermost level carries the C const)
        core = ("*const " if const and k == 0 else "*mut ") + core
    return core


def split_decl(decl):
    """'const uint8_t r[32]' -> ('const uint8_t', 'r', ['32']);  'zk_params** out' -> ('zk_params**', 'out', [])"""
    decl = decl.strip()
    dims = re.findall(r"\[([^\]]*)\]", decl)
    decl = re.sub(r"\[[^\]]*\]", "", decl).strip()
    m = re.fullmatch(r"(.*?)([A-Za-z_][A-Za-z0-9_]*)", decl)
    ctype, name = m.group(1).strip(), m.group(2)
    ctype = re.sub(r"\s*\*", "*", ctype)
    return ctype, name, dims


def field_lines(body):
    out = []
    bytes_before = 0   # of the fields so far while they are all uint8_t (scalars or arrays with literal bounds), else None
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        first, *rest = [x.strip() for x in stmt.split(",")]
        ctype, name, dims = split_decl(first)
        decls = [(name, dims)]
        for r in rest:
            dims_r = re.findall(r"\[([^\]]*)\]", r)
            decls.append((re.sub(r"\[[^\]]*\]", "", r).strip(), dims_r))
        for name, dims in decls:
            if dims:
                t = base_type(ctype)
                for d in reversed(dims):
                    t = "[%s; %s]" % (t, rust_expr(d))
            else:
                t = param_type(ctype, [])
            if ctype in ("uint16_t", "int64_t"):
                assert not dims and (ctype == "int64_t" or (bytes_before is not None and bytes_before % 2 == 0)), \
                    "a uint16_t as [u8; 2] keeps its offset only at the head of a struct or behind an even number of bytes"
                out.append("    // %s is %s in the header" % (name, {"uint16_t": "a little-endian uint16_t", "int64_t": "an int64_t, two's complement"}[ctype]))
            out.append("    pub %s: %s," % (name, t))
            if bytes_before is not None and ctype == "uint8_t" and all(d.strip().isdigit() for d in dims):
                size = 1
                for d in dims:
                    size *= int(d)
                bytes_before += size
            else:
                bytes_before = None
    return out


def generate():
    raw = open(HEADER).read()
    src = strip_comments(raw)
    o = []
    o.append("// GENERATED by tools/gen_rust_bindings.py from include/zkamd.h - do not edit; regenerate.")
    o.append("// The whole C boundary of libzkamd.so as a Rust `extern \"C\"` block: what core/proofs would add as")
    o.append("// src/zkamd_sys.rs (INTEGRATION.md).  Not compiled in this image (no rustc); kept in step with the header by")
    o.append("// tests/test_abi.py.  Contracts, units and the reference file:line each entry replaces: include/zkamd.h.")
    o.append("#![allow(non_camel_case_types, dead_code)]")
    o.append("use std::os::raw::{c_char, c_int, c_void};")
    o.append("")
    o.append("pub type zk_status = i32;")
    # constants: the anonymous enums and the #defines
    for m in re.finditer(r"enum\s*\{(.*?)\};", src, flags=re.S):
        names = re.findall(r"(ZK_[A-Z_0-9]+)\s*=\s*(\d+)", m.group(1))
        ty = "zk_status" if any(n == "ZK_OK" for n, _ in names) else "u8"
        for n, v in names:
            o.append("pub const %s: %s = %s;" % (n, ty, v))
    for n, v in re.findall(r"^#define\s+(ZK_[A-Z_0-9]+)\s+(0x[0-9A-Fa-f]+|\d+)u?\s*$", src, flags=re.M):
        ty = "usize" if n in ("ZK_ANONYMOUS_SIZE",) else "u32"
        o.append("pub const %s: %s = %s;" % (n, ty, v))
    o.append("")
    # opaque handles
    for n in sorted(set(re.findall(r"typedef struct (zk_[a-z0-9_]+) \1;", src))):
        o.append("#[repr(C)]")
        o.append("pub struct %s {" % n)
        o.append("    _opaque: [u8; 0],")
        o.append("}")
    o.append("")
    # plain structs
    for m in re.finditer(r"typedef struct\s*\{(.*?)\}\s*(zk_[a-z0-9_]+);", src, flags=re.S):
        o.append("#[repr(C)]")
        o.append("#[derive(Clone, Copy)]")
        o.append("pub struct %s {" % m.group(2))
        o.extend(field_lines(m.group(1)))
        o.append("}")
    o.append("")
    o.append("#[link(name = \"zkamd\")]")
    o.append("extern \"C\" {")
    protos = re.findall(r"^([a-zA-Z_][a-zA-Z0-9_ \*]*?)\b(zk_[a-z0-9_]+)\s*\(([^;]*?)\);", src, flags=re.M | re.S)
    for ret, name, params in protos:
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        ps = []
        params = " ".join(params.split())
        if params != "void":
            for p in params.split(","):
                ctype, pname, dims = split_decl(p)
                if pname in ("type", "in", "ref", "box", "fn", "mod", "move", "match", "loop"):
                    pname += "_"
                ps.append("%s: %s" % (pname, param_type(ctype, dims)))
        rt = "" if ret == "void" else " -> " + param_type(ret, [])
        line = "    pub fn %s(%s)%s;" % (name, ", ".join(ps), rt)
        if len(line) > 124:   # one parameter per line
            line = "    pub fn %s(\n%s\n    )%s;" % (name, "\n".join("        %s," % p for p in ps), rt)
        o.append(line)
    o.append("}")
    return "\n".join(o) + "\n", [n for _, n, _ in protos]


def main():
    text, _ = generate()
    if "--check" in sys.argv:
        have = open(OUT).read() if os.path.exists(OUT) else ""
        if have != text:
            print("include/zkamd_sys.rs is out of date: run python tools/gen_rust_bindings.py")
            return 1
        return 0
    open(OUT, "w").write(text)
    print("wrote", OUT, len(text.splitlines()), "lines")
    return 0


if __name__ == "__main__":
    sys.exit(main())
