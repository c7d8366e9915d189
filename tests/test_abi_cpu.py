"""CPU-side checks of the C-ABI boundary: the library builds/loads without a GPU and exports every
symbol include/vct_hip.h declares (no compute calls here); the ctypes mirror of the header (structs, signatures, constants)
agrees with the C compiler's reading of it."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vct_hip.h")


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()
    from vct_amd import _lib
    return _lib.LIB_PATH


def declared_symbols():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vct_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported(lib_path):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    decl = declared_symbols()
    assert len(decl) >= 17
    missing = [s for s in decl if s not in exported]
    assert not missing, missing


def test_binding_covers_header(lib_path):
    from vct_amd import _lib
    assert sorted(set(declared_symbols())) == sorted(set(_lib.exported_symbols()))
    lib = _lib.load()
    assert lib.vct_abi_version() == _lib.ABI_VERSION == 16
    buf = ctypes.create_string_buffer(128)
    assert lib.vct_build_info(buf, 128) > 0 and b"gfx950" in buf.value


def test_argument_errors_are_codes_not_crashes(lib_path):
    """Null descriptors / bad enums return VCT_E_* (negative) without touching a device."""
    from vct_amd import _lib
    lib = _lib.load()
    assert lib.vct_gemm(None, None) == -1
    d = _lib.GemmDesc()
    assert lib.vct_gemm(d, None) == -1                      # null pointers
    assert lib.vct_attn_fwd(None, None) == -1
    assert lib.vct_cast(7, 0, None, None, 10, None) == -1   # bad dtype enum
    assert lib.vct_ln_ws_rows(4864) > 0
    with pytest.raises(ValueError):
        _lib.check(-2, "x")
    with pytest.raises(RuntimeError):
        _lib.check(700, "x")


def test_gemm_last_route_is_zero_before_any_gemm(lib_path):
    """vct_gemm_last_route: a host-side record; all zero before this thread ran a GEMM (a refused descriptor records nothing), and a
    buffer shorter than the record is refused."""
    import threading
    from vct_amd import _lib
    lib = _lib.load()
    n = _lib.GEMM_ROUTE_INTS
    assert n == 17
    got = {}

    def fresh_thread():                                    # the record is thread-local: a new thread has run no GEMM whatever ran before
        buf = (ctypes.c_int32 * n)(*([7] * n))
        assert lib.vct_gemm(_lib.GemmDesc(), None) == -1   # refused before any launch
        got["rc"] = lib.vct_gemm_last_route(buf, n)
        got["rec"] = list(buf)
        short = (ctypes.c_int32 * n)(*([7] * n))
        got["short"] = (lib.vct_gemm_last_route(short, n - 1), list(short))
        got["null"] = lib.vct_gemm_last_route(None, n)
    t = threading.Thread(target=fresh_thread)
    t.start(); t.join()
    assert got["rc"] == 0 and got["rec"] == [0] * n
    assert got["short"] == (-1, [7] * n) and got["null"] == -1


def test_new_entry_points_validate_arguments(lib_path):
    from vct_amd import _lib
    lib = _lib.load()
    assert lib.vct_gemm_grouped(None, 3, None) == -1
    arr = (_lib.GemmDesc * 9)()
    assert lib.vct_gemm_grouped(arr, 9, None) == -1                    # more than VCT_GEMM_GROUP_MAX problems
    assert lib.vct_gemm_grouped(arr, 2, None) == -1                    # null operands inside the descriptors
    assert lib.vct_gemm_grouped_workspace_bytes(arr, 2, 5) == 0
    assert lib.vct_greedy_select(1, 4, 10, None, 16, None, 1, 102, None, None, None, 3, None) == -1
    assert lib.vct_gather_pad_rows(0, 4, 3, 16, None, None, None, None, None, None) == -1
    assert lib.vct_warm(None, 64, None) == -1 and lib.vct_warm(ctypes.c_void_p(16), 8, None) == -2
    assert lib.vct_add_ln_ln_bwd(1, 8, 64, *([None] * 15), 0, 0.0, None) == -1


# ---- the hand-written ctypes mirror (vct_amd/_lib.py) against the header, exhaustively: every struct field, every signature, every
# constant.  Two gcc runs on the header; the library is not needed. ---------------------------------------------------------------
def _mirror_structs():
    from vct_amd import _lib
    return [v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure]


def _layout(S, c_expr=False):
    """{"T": sizeof, "T.f offset": offset, "T.f size": size, ...} of the ctypes mirror S of the C struct T -- or, with c_expr, the C
    expressions of the same numbers."""
    T, fields = S._c_name_, [f[0] for f in S._fields_]
    if c_expr:
        return {T: f"sizeof({T})", **{f"{T}.{f} offset": f"offsetof({T}, {f})" for f in fields},
                **{f"{T}.{f} size": f"sizeof((({T}*)0)->{f})" for f in fields}}
    return {T: ctypes.sizeof(S), **{f"{T}.{f} offset": getattr(S, f).offset for f in fields},
            **{f"{T}.{f} size": getattr(S, f).size for f in fields}}


def _layout_mismatches(S, from_c):
    """The entries of S's layout ("struct", "struct.field offset", "struct.field size") that are not the C compiler's."""
    return [k for k, v in _layout(S).items() if from_c.get(k) != v]


@pytest.fixture(scope="module")
def from_c(tmp_path_factory):
    """One C program against the header prints every C_CONSTANTS name and the layout of every mirrored struct: {name: number}."""
    from vct_amd import _lib
    exprs = {k: k for k in _lib.C_CONSTANTS}
    for S in _mirror_structs():
        if "_c_name_" in S.__dict__:                       # (a mirror without a name fails test_every_struct_field_... by name)
            exprs.update(_layout(S, c_expr=True))
    d = tmp_path_factory.mktemp("abi")
    (d / "abi.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vct_hip.h"\nint main(void) {\n'
                             + "".join(f'  printf("%lld\\n", (long long)({e}));\n' for e in exprs.values()) + "  return 0;\n}\n")
    subprocess.run(["gcc", "-I", os.path.dirname(HDR), str(d / "abi.c"), "-o", str(d / "abi")], check=True)
    out = subprocess.run([str(d / "abi")], capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == len(exprs)
    return dict(zip(exprs, map(int, out)))


def test_every_struct_field_matches_the_c_header(from_c):
    """Every ctypes.Structure of _lib names its C struct, every typedef struct of the header has a mirror, and sizeof of each struct
    and offsetof + sizeof of each field (arrays and nested structs included) are the C compiler's."""
    structs = _mirror_structs()
    unnamed = [S.__name__ for S in structs if "_c_name_" not in S.__dict__]
    assert not unnamed, f"ctypes mirrors without _c_name_: {unnamed}"
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert sorted(S._c_name_ for S in structs) == sorted(re.findall(r"typedef\s+struct\s+(\w+)", hdr))
    bad = [k for S in structs for k in _layout_mismatches(S, from_c)]
    assert not bad, f"ctypes layout differs from the header at: {bad}"
    assert len(structs) >= 25 and sum(len(S._fields_) for S in structs) >= 489


_SCALARS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "uint32_t": "u32", "float": "f32", "double": "f64"}


def _c_type(s):
    """Class of a C type as gcc prints it: i32 / i64 / u32 / f32 / f64, "ptr:<pointee>", anything else as spelled."""
    s = s.replace("const ", "").strip()
    if "(*)" in s:
        return "ptr:fn"
    return "ptr:" + _c_type(s[:-1]) if s.endswith("*") else _SCALARS.get(s, s)


def _py_type(t):
    """The same class of a ctypes type; c_void_p / c_char_p are the untyped "ptr", which stands for any C pointer."""
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p):
        return "ptr"
    if issubclass(t, ctypes.Structure):
        return t._c_name_
    if issubclass(t, ctypes._Pointer):
        return "ptr:" + _py_type(t._type_)
    return {ctypes.c_int32: "i32", ctypes.c_int64: "i64", ctypes.c_uint32: "u32", ctypes.c_float: "f32", ctypes.c_double: "f64"}[t]


def _sig_mismatches(name, sig, proto):
    """What differs between a _SIGS entry (restype, argtypes) and the header's prototype (return type, [argument types]), by
    position.  POINTER(S) needs the C pointee S._c_name_; a struct pointer in C needs POINTER of its mirror or plain c_void_p."""
    def same(py, c):
        return py == c or (py.endswith("ptr") and c.startswith(py + ":"))
    bad = [] if same(_py_type(sig[0]), _c_type(proto[0])) else [f"{name}: returns {proto[0]} in C, {_py_type(sig[0])} in ctypes"]
    if len(sig[1]) != len(proto[1]):
        return bad + [f"{name}: {len(proto[1])} arguments in C, {len(sig[1])} in ctypes"]
    return bad + [f"{name}: argument {i}: {c} in C, {_py_type(a)} in ctypes" for i, (a, c) in enumerate(zip(sig[1], proto[1]))
                  if not same(_py_type(a), _c_type(c))]


def test_every_signature_matches_the_c_header(tmp_path):
    """gcc's own reading of the header (-aux-info: one normalised prototype per function) against _SIGS: the same functions, and
    for each the return type, the number of arguments and every argument's class."""
    from vct_amd import _lib
    (tmp_path / "tu.c").write_text('#include "vct_hip.h"\n')
    subprocess.run(["gcc", "-fsyntax-only", "-aux-info", str(tmp_path / "tu.X"), "-I", os.path.dirname(HDR), str(tmp_path / "tu.c")], check=True)
    protos = {}
    for ret, name, args in re.findall(r"extern (.+?)\b(vct_\w+) \((.*)\);", (tmp_path / "tu.X").read_text()):
        protos[name] = (ret.strip(), [] if args == "void" else args.split(", "))
    assert sorted(protos) == sorted(_lib._SIGS) and len(protos) >= 102
    bad = [m for name, sig in _lib._SIGS.items() for m in _sig_mismatches(name, sig, protos[name])]
    assert not bad, bad


def test_constants_match_the_c_header(from_c):
    from vct_amd import _lib
    bad = {k: (v, from_c[k]) for k, v in _lib.C_CONSTANTS.items() if from_c[k] != v}
    assert not bad, f"name: (_lib, header) {bad}"
    assert len(_lib.C_CONSTANTS) >= 39 and _lib.C_CONSTANTS["VCT_ABI_VERSION"] == 16


def test_the_mirror_checks_can_fail(from_c):
    """Wrong mirrors of vct_adam_range (two fields swapped; a field of the wrong width) and a wrong signature (int64_t where the
    header has float) are reported, by name."""
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p

    class Swapped(ctypes.Structure):
        _c_name_ = "vct_adam_range"
        _fields_ = [("begin", i64), ("end", i64), ("shadow", i32), ("blk0", i32)]

    class Narrow(ctypes.Structure):
        _c_name_ = "vct_adam_range"
        _fields_ = [("begin", i32), ("end", i64), ("blk0", i32), ("shadow", i32)]
    assert _layout_mismatches(Swapped, from_c) == ["vct_adam_range.shadow offset", "vct_adam_range.blk0 offset"]
    assert _layout_mismatches(Narrow, from_c) == ["vct_adam_range.begin size"]
    scale = ("int", ["float *", "int64_t", "float", "void *"])             # vct_scale as gcc prints it
    assert _sig_mismatches("vct_scale", (ctypes.c_int, [vp, i64, ctypes.c_float, vp]), scale) == []
    assert _sig_mismatches("vct_scale", (ctypes.c_int, [vp, i64, i64, vp]), scale) == ["vct_scale: argument 2: float in C, i64 in ctypes"]
    assert _sig_mismatches("vct_scale", (i64, [vp, i64, vp]), scale) == ["vct_scale: returns int in C, i64 in ctypes",
                                                                         "vct_scale: 4 arguments in C, 3 in ctypes"]
    gemm = ("int", ["const vct_gemm_desc *", "void *"])
    assert _sig_mismatches("vct_gemm", (ctypes.c_int, [ctypes.POINTER(Swapped), vp]), gemm) == [
        "vct_gemm: argument 0: const vct_gemm_desc * in C, ptr:vct_adam_range in ctypes"]


def test_layer_ss_entry_points_validate_arguments(lib_path):
    """Sample-stationary layer forward (csrc/vct_layer_ss.hip): shape predicate, stream length and argument errors as codes."""
    from vct_amd import _lib
    lib = _lib.load()
    assert lib.vct_layer_ss_supported(_lib.BF16, 512, 8, 2048, 19, 13) == 1
    assert lib.vct_layer_ss_supported(_lib.BF16, 512, 8, 2048, 13, 0) == 1
    assert lib.vct_layer_ss_supported(_lib.F32, 512, 8, 2048, 19, 13) == 0          # parity mode stays on the unfused kernels
    assert lib.vct_layer_ss_supported(_lib.BF16, 768, 8, 2048, 19, 13) == 0
    assert lib.vct_layer_ss_supported(_lib.BF16, 512, 8, 2048, 33, 13) == 0 and lib.vct_layer_ss_supported(_lib.BF16, 512, 8, 2048, 19, 17) == 0
    assert lib.vct_layer_ss_supported(_lib.BF16, 512, 8, 1000, 19, 13) == 0
    assert lib.vct_layer_ss_stream_chunks(2048, 0) == 96 and lib.vct_layer_ss_stream_chunks(2048, 1) == 128     # 6.3 MB / 8.4 MB of bf16
    assert lib.vct_layer_ss_fwd(None, 1, None) == -1
    d = _lib.LayerSsDesc()
    d.dtype, d.B, d.L, d.d, d.H, d.ff = _lib.BF16, 4, 13, 512, 8, 2048
    d.nchunks = 96
    assert lib.vct_layer_ss_fwd(d, 1, None) == -1                                   # null operands
    d.nchunks = 95
    assert lib.vct_layer_ss_fwd(d, 1, None) in (-1, -2)                            # (stream length does not match the layer)
    assert lib.vct_ss_pack(None, 1, None, None) == -1
    # the backward of a self-attention + feed-forward stack (csrc/vct_layer_ss_bwd.hip)
    assert lib.vct_layer_ss_bwd_stream_chunks(2048) == 96 and lib.vct_layer_ss_bwd_stream_chunks(512) == 48
    assert lib.vct_layer_ss_bwd(None, 1, None) == -1
    q = _lib.LayerSsBwdDesc()
    q.dtype, q.B, q.L, q.d, q.H, q.ff, q.nchunks = _lib.BF16, 4, 13, 512, 8, 2048, 96
    assert lib.vct_layer_ss_bwd(q, 1, None) == -1                                   # null operands
    assert lib.vct_layer_ss_bwd(q, 5, None) == -2                                   # more layers than one launch carries
    q.d = 768
    assert lib.vct_layer_ss_bwd(q, 1, None) == -2
    # Adam that also maintains stream-order packed weight copies: a table without a shadow / a misaligned base are argument errors
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    assert lib.vct_adam_step_pk(p, p, p, p, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, p, 0, 0, 0, None, p, 1, 0, None) == -1
    assert lib.vct_adam_step_pk(p, p, p, p, p, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, p, 0, 0, 0, None, p, 1, 2, None) == -1
    assert lib.vct_adam_step_pk(p, p, p, p, p, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, p, 0, 0, 0, None, None, -1, 0, None) == -1


def test_decode_block_entry_refuses_before_any_launch(lib_path):
    """vct_decode_block (csrc/vct_decode_block.hip): unsupported shapes, a missing res, LayerNorm 2 without LayerNorm 1 and
    misaligned vector inputs are codes.  Dummy host pointers; every descriptor also carries a later refusal with ANOTHER code
    (null part_out: VCT_E_ARG; generator with V = 0: VCT_E_SHAPE), so a missing check shows as the wrong code, not as a launch."""
    from vct_amd import _lib
    lib = _lib.load()
    ARG, SHAPE, ALIGN = -1, -2, -3
    raw = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(raw) + 15) & ~15          # 16-byte aligned; p + 4 is not, p + 8 is 8- but not 16-byte aligned

    def call(kind, **kw):
        q = _lib.DecodeBlockDesc()
        q.kind, q.d, q.ff, q.V, q.Lk = kind, 512, 64, 127, 1
        q.res, q.w_a, q.ld_a, q.b_a, q.w_b, q.ld_b = p, p, 512, p, p, 512
        q.slot, q.kc, q.vc, q.kv_ld = p, p, p, 1536
        q.part_out = None
        for k, v in kw.items():
            setattr(q, k, v)
        return lib.vct_decode_block(q, None)
    assert lib.vct_decode_block(None, None) == ARG and call(4) == ARG and call(-1) == ARG
    assert call(2) == ARG                                                       # (the guard itself: null part_out)
    # shapes
    assert call(2, part=p, n_part=33) == SHAPE and call(2, part=p, n_part=32) == ARG
    assert call(2, ff=2112) == SHAPE and call(2, ff=96) == SHAPE and call(2, ff=0) == SHAPE and call(2, ff=2048) == ARG
    for kind in (0, 1):
        assert call(kind, Lk=0) == SHAPE and call(kind, Lk=65) == SHAPE and call(kind, Lk=64) == ARG
    for kind in range(4):
        assert call(kind, d=768) == SHAPE and call(kind, d=0) == SHAPE
    assert call(3, V=0, part_out=p) == SHAPE and call(3, V=-5, part_out=p) == SHAPE
    # the input vector: res is required whenever id is absent (the kernels load it unconditionally) ...
    guard = dict(V=0, part_out=p)                                               # generator with V = 0: VCT_E_SHAPE at the very end
    assert call(3, res=None, **guard) == ARG
    assert call(3, res=None, part=p, n_part=8, **guard) == ARG                  # (partial vectors alone were accepted before)
    assert call(3, res=None, res_bias=p, **guard) == ARG
    assert call(3, id=p, res=None, **guard) == ARG and call(3, id=p, table=p, res=None, **guard) == ARG     # id needs table and pos_row
    assert call(3, id=p, table=p, pos_row=p, res=None, **guard) == SHAPE        # a complete embed source passes on to the guard
    # ... LayerNorm parameters come in pairs, the second only after the first
    assert call(3, g2=p, b2=p, **guard) == ARG and call(3, g1=p, **guard) == ARG and call(3, g1=p, b1=p, g2=p, **guard) == ARG
    assert call(3, g1=p, b1=p, g2=p, b2=p, **guard) == SHAPE
    # ... and every vector input is read as 16-byte loads
    for off in (4, 8):
        assert call(2, res=p + off) == ALIGN
        assert call(2, res_bias=p + off) == ALIGN
        assert call(2, part=p + off, n_part=8) == ALIGN
        assert call(2, id=p, table=p + off, pos_row=p) == ALIGN
        assert call(2, id=p, table=p, pos_row=p + off) == ALIGN
    assert call(2, res_bias=p, part=p, n_part=8) == ARG                         # all aligned: on to the guard
    # the selection workspace holds 8-byte pairs
    sel = dict(tok_out=p, ended=p, ended_count=p, all_ended_at=p, t=3)
    assert call(3, sel_ws=p + 4, **sel) == ALIGN and call(3, sel_ws=p + 8, **sel) == ARG
    assert call(3, sel_ws=p, tok_out=p, ended=p, ended_count=p, t=3, **guard) == ARG     # selection without all_ended_at
    assert call(3, sel_ws=p, **sel, **guard) == SHAPE


def test_no_cpu_fallback_when_library_is_missing(monkeypatch, lib_path):
    from vct_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libvct_hip.so")
    with pytest.raises(RuntimeError, match="no CPU/eager fallback"):
        _lib.load()


def test_runtime_entry_points_validate_arguments(lib_path):
    """Launch lists / sync points / taps (csrc/vct_runtime.hip): argument errors are codes; an empty recording works
    without a device."""
    from vct_amd import _lib
    lib = _lib.load()
    assert lib.vct_cmdlist_create(None) == -1
    h = ctypes.c_void_p()
    assert lib.vct_cmdlist_create(ctypes.byref(h)) == 0 and h.value
    assert lib.vct_cmdlist_end(h) == -1                      # not recording
    assert lib.vct_cmdlist_begin(h, None) == 0
    assert lib.vct_cmdlist_begin(h, None) == -1              # one recording per thread
    assert lib.vct_cmdlist_replay(h, None) == -1             # still recording
    assert lib.vct_cmdlist_end(h) == 0
    assert lib.vct_cmdlist_size(h) == 0 and lib.vct_cmdlist_streams(h) == 1
    assert lib.vct_cmdlist_replay(h, None) == 0              # nothing to issue
    assert lib.vct_cmdlist_destroy(h) == 0
    assert lib.vct_sync_record(64, None) == -1 and lib.vct_sync_wait(-1, None) == -1
    assert lib.vct_stream_wait(None, None) == 0              # same stream: no edge needed
    assert lib.vct_tap(24, 0, None) == -1 and lib.vct_tap(0, 2, None) == -1
    assert lib.vct_tap(0, 0, None) == 0                      # taps disabled: no-op
    assert lib.vct_tap_collect(0, None, 0) == 0


def test_replay_reports_the_first_failed_command(lib_path):
    """A command of a recorded list cannot return a status to the call that recorded it: the first non-zero status of a replay
    (failed RCCL collective, event record / wait, memset) must come back from vct_cmdlist_replay.  vct_cmdlist_inject_status is
    the fault-injection hook of that path (host commands, which need a device to drain a stream: tests/test_executor_gpu.py)."""
    from vct_amd import _lib
    lib = _lib.load()
    assert lib.vct_cmdlist_inject_status(0, None) == 0 and lib.vct_cmdlist_inject_status(10005, None) == 10005      # eager
    assert lib.vct_cmdlist_host_call(None, None, None) == -1
    h = ctypes.c_void_p()
    assert lib.vct_cmdlist_create(ctypes.byref(h)) == 0
    assert lib.vct_cmdlist_begin(h, None) == 0
    assert lib.vct_cmdlist_inject_status(0, None) == 0
    assert lib.vct_cmdlist_inject_status(10003, None) == 0        # recorded, not reported now
    assert lib.vct_cmdlist_inject_status(10007, None) == 0
    assert lib.vct_cmdlist_end(h) == 0
    assert lib.vct_cmdlist_size(h) == 3
    assert lib.vct_cmdlist_replay(h, None) == 10003               # the FIRST failure, sticky over the rest of the replay
    with pytest.raises(RuntimeError, match="ncclResult_t 3"):
        _lib.check(lib.vct_cmdlist_replay(h, None), "replay")
    assert lib.vct_cmdlist_begin(h, None) == 0 and lib.vct_cmdlist_end(h) == 0
    assert lib.vct_cmdlist_replay(h, None) == 0                   # a fresh (empty) recording: no stale status
    assert lib.vct_cmdlist_destroy(h) == 0
