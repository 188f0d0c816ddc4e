"""CPU checks of the binding that statecatcher_amd/_lib.py derives from include/statecatcher.h:
the parser on small header texts, the real header against literal signatures, struct layouts and
constants (the same layout numbers capi.cpp static_asserts), and the per-launch job caps that
ops.py honours."""
import ctypes

import pytest
import torch

from statecatcher_amd import _lib, ops

I, L, Z, F, D, P, S = (ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float,
                       ctypes.c_double, ctypes.c_void_p, ctypes.c_char_p)


# ------------------------------------------------------------------ parser, inline texts -----
def test_parser_ignores_comments_and_wrappers():
    consts, structs, sigs = _lib.parse_header("""
        /* sc_fake(gates_ptr, h0_ptr) in a comment; int sc_fake2(int a); and sc_mlstm_*_io */
        #ifndef X_H
        #define X_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        // int sc_fake3(void);
        int sc_one(void);   // trailing int sc_fake4(void);
        int sc_two();
        #ifdef __cplusplus
        }
        #endif
        #endif /* X_H */
        """)
    assert sigs == {"sc_one": (I, []), "sc_two": (I, [])}
    assert list(sigs) == ["sc_one", "sc_two"] and consts == {} and structs == {}


def test_parser_maps_every_supported_type():
    _, structs, sigs = _lib.parse_header("""
        typedef struct { float* p; int64_t n; } sc_t;
        const char* sc_msg(void);
        void sc_nothing(int a);
        size_t sc_bytes(size_t n, double x, float y, int64_t z);
        int64_t sc_count(const sc_t* t, const struct sc_t *u, int nt);
        int sc_out(int B, int* t_blocks, const int64_t* lens, int32_t* tokens, void* stream,
                   const void *w, const float* const_like);
        int sc_unnamed(int, float*);
        """)
    assert sigs == {"sc_msg": (S, []), "sc_nothing": (None, [I]), "sc_bytes": (Z, [Z, D, F, L]),
                    "sc_count": (L, [P, P, I]), "sc_out": (I, [I, P, P, P, P, P, P]),
                    "sc_unnamed": (I, [I, P])}
    assert structs["sc_t"]._fields_ == [("p", P), ("n", L)]


def test_parser_structs_both_typedef_forms_and_multi_declarators():
    _, structs, _ = _lib.parse_header("""
        typedef struct {
          const float* w;
          int64_t ld, rows, D;
        } sc_a;
        typedef struct sc_b {
          const void* st;
          int B, N;
          const float *lnz_w, *lnz_b, *lnh_w, *lnh_b;
          float eps;
        } sc_b;
        """)
    a, b = structs["sc_a"], structs["sc_b"]
    assert issubclass(a, ctypes.Structure) and a.__name__ == "sc_a"
    assert a._fields_ == [("w", P), ("ld", L), ("rows", L), ("D", L)]
    assert b._fields_ == [("st", P), ("B", I), ("N", I), ("lnz_w", P), ("lnz_b", P), ("lnh_w", P),
                          ("lnh_b", P), ("eps", F)]
    assert ctypes.sizeof(a) == 32 and ctypes.sizeof(b) == 56 and b.eps.offset == 48


def test_parser_constants():
    consts, _, _ = _lib.parse_header("""
        #define SC_EINVAL (-1)
        #define SC_F16 2   /* half */
        #define SC_NEG -3
        #define SC_PAREN ( 16 )
        #define OTHER_GUARD_H
        """)
    assert consts == {"SC_EINVAL": -1, "SC_F16": 2, "SC_NEG": -3, "SC_PAREN": 16}


@pytest.mark.parametrize("text,quoted", [
    ("int sc_f(unsigned n);", "unsigned n"),
    ("int sc_f(unsigned int n);", "unsigned int n"),
    ("unsigned sc_f(int n);", "unsigned sc_f(int n);"),
    ("int sc_f(long n);", "long n"),
    ("long sc_f(void);", "long sc_f(void);"),
    ("int sc_f(long long n);", "long long n"),
    ("typedef struct { int a[4]; } sc_t;", "int a[4]"),
    ("int sc_f(float x[3]);", "int sc_f(float x[3]"),
    ("int sc_ok(void); stray tokens int sc_g(void);", "stray tokens int sc_g(void);"),
    ("int sc_ok(void); garbage", "garbage"),
    ("int sc_f(void (*cb)(int));", "int sc_f(void (*cb)(int))"),
    ("int sc_f(void* p, void v);", "void v"),
    ("float* sc_f(void);", "float* sc_f(void);"),
    ("int sc_f(sc_unknown_job* j);", "sc_unknown_job* j"),
    ("typedef struct sc_x { int a; } sc_y;", "typedef struct sc_x { int a; } sc_y;"),
    ("typedef struct { int; } sc_t;", "typedef struct { int; } sc_t;"),
    ("int sc_f(int a,, int b);", "int sc_f(int a,, int b);"),
    ('extern "C" {\nint sc_f(void);', "extern"),
    ("#define SC_RATE 1.5", "SC_RATE 1.5"),
    ("#define SC_MANY (1 << 4)", "SC_MANY (1 << 4)"),
    ("#define SC_TWO_LINES \\\n 4", "SC_TWO_LINES"),
])
def test_parser_fails_closed(text, quoted):
    with pytest.raises(ValueError) as e:
        _lib.parse_header(text)
    assert quoted in str(e.value)


def test_missing_header_names_the_path(monkeypatch, tmp_path):
    gone = str(tmp_path / "include" / "statecatcher.h")
    monkeypatch.setattr(_lib, "HEADER_PATH", gone)
    with pytest.raises(RuntimeError, match="header missing") as e:
        _lib._read_header()
    assert gone in str(e.value)


# ------------------------------------------------------------------ the real header ----------
# copied from the hand-written table this binding replaced (ABI 14)
SIGNATURES = {
    "sc_last_error": (S, []),
    "sc_lucy_scan_ckpt_numel": (L, [I, I, I]),
    "sc_ctc_workspace_bytes": (Z, [I, I, I]),
    "sc_fbank": (I, [P, I, L, L, I, F, P, P, Z, P]),
    "sc_adam_step": (I, [P, I, P, L, D, D, D, D, D, D, I, D, D, P, P]),
    "sc_mlstm_bwd_io": (I, [P, P, P, I, I, P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, F, P, P, P, P,
                            P, P, P, P, P]),
    "sc_rnnt_joint_geometry": (I, [I, I, I, I, P, P, P]),
    "sc_lucy_frame_gemm_multi": (I, [I, I, F, P, I, P]),
    "sc_ctc_beam_frames": (I, [P, I, I, I, I, I, L, L, P, P, L, L, I, I, I, P, Z, P, Z, P]),
}

# class, header name, sizeof, last field, its offset (capi.cpp static_asserts the same numbers),
# field names
STRUCTS = [
    ("AdamTensor", "sc_adam_tensor", 40, "n", 32, "p g m v n"),
    ("ImageJob", "sc_image_job", 80, "row_shift", 72,
     "src dst dst_t rows cols cols_pad ld_src block_d col_scale row_shift"),
    ("LnFoldJob", "sc_ln_fold_job", 80, "D", 72,
     "w gamma beta bias shift bias_out rowsum ld rows D"),
    ("FrameGemmJob", "sc_frame_gemm_job", 144, "mask", 136,
     "x ldx K ln_w ln_b st_in nst_in w ldw bias B N y ldy st_out z st_z s mask"),
    ("FrameCellJob", "sc_frame_cell_job", 120, "D", 116,
     "z st_z nst_z hp st_h nst_h lnz_w lnz_b lnh_w lnh_b h out ldo mask B D"),
    ("TFrameJob", "sc_tframe_job", 136, "mask", 128,
     "x ldx K ln_w ln_b st_in nst_in w ldw bias B D h s out ldo st_out mask"),
]


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_header_signature_matches_literal(name):
    assert _lib._SIGS[name] == SIGNATURES[name]


def test_header_is_fully_bound():
    assert len(_lib.EXPORTED) >= 86 and all(n.startswith("sc_") for n in _lib.EXPORTED)
    assert sorted(_lib.STRUCTS) == sorted(s[1] for s in STRUCTS)


@pytest.mark.parametrize("cls,cname,size,last,offset,names", STRUCTS, ids=[s[0] for s in STRUCTS])
def test_struct_layout(cls, cname, size, last, offset, names):
    c = getattr(_lib, cls)
    assert c is _lib.STRUCTS[cname] and issubclass(c, ctypes.Structure)
    assert [n for n, _ in c._fields_] == names.split()
    assert ctypes.sizeof(c) == size
    assert c._fields_[-1][0] == last and getattr(c, last).offset == offset


def test_constants_equal_their_literals():
    want = dict(SC_EINVAL=-1, SC_F32=0, SC_BF16=1, SC_F16=2, SC_ABI_VERSION=14,
                SC_MAX_FRAME_JOBS=8, SC_MAX_IMAGE_JOBS=16, SC_MAX_FOLD_JOBS=16,
                SC_FRAME_PLAIN=0, SC_FRAME_STATS=1, SC_FRAME_CELL_UNFUSED=2, SC_FRAME_CELL_FUSED=3,
                SC_STEP_FUSED=0, SC_STEP_UNFUSED_A=1, SC_STEP_UNFUSED_B=2,
                SC_FBANK_MFCC=0, SC_FBANK_MEL=1)
    assert _lib.CONSTANTS == want
    for k, v in want.items():
        assert getattr(_lib, k) == v
    assert _lib.ABI_VERSION == 14
    assert _lib._DTYPE == {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
    assert (ops.FRAME_PLAIN, ops.FRAME_STATS, ops.FRAME_CELL_UNFUSED, ops.FRAME_CELL_FUSED) == \
        (0, 1, 2, 3)
    assert (ops.STEP_FUSED, ops.STEP_UNFUSED_A, ops.STEP_UNFUSED_B) == (0, 1, 2)


# ------------------------------------------------------------------ per-launch job caps ------
class StubLib:
    """Stands in for the loaded library: records (name, leading scalars, job-array type and
    length, njobs, stream) of every call and returns success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            *scalars, jobs, njobs, stream = args
            self.calls.append((name, tuple(scalars), type(jobs)._type_, len(jobs), njobs, stream))
            return 0
        return fn


@pytest.fixture
def stub(monkeypatch):
    lib = StubLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(ops, "require_device", lambda *t: None)   # the stub launches nothing
    monkeypatch.setattr(ops, "stream_of", lambda t: "stream")
    return lib


def sizes(stub, name):
    assert all(c[3] == c[4] for c in stub.calls)
    return [c[3] for c in stub.calls if c[0] == name]


def test_chunked_launch_helper(stub):
    jobs = [_lib.TFrameJob() for _ in range(17)]
    ops._launch_jobs("sc_any", _lib.TFrameJob, 8, jobs, "st", 1, 2.0)
    assert stub.calls == [("sc_any", (1, 2.0), _lib.TFrameJob, n, n, "st") for n in (8, 8, 1)]
    stub.calls.clear()
    ops._launch_jobs("sc_any", _lib.TFrameJob, 8, [], "st")
    assert stub.calls == []
    ops._launch_jobs("sc_any", _lib.TFrameJob, 8, jobs[:8], "st")
    assert sizes(stub, "sc_any") == [8]


def test_frame_loops_honour_the_cap(stub):
    for n, want in ((17, [8, 8, 1]), (0, [])):
        stub.calls.clear()
        ops.lucy_frame_gemm_multi(ops.FRAME_STATS, torch.bfloat16,
                                  [_lib.FrameGemmJob() for _ in range(n)], "st", eps=0.5)
        ops.lucy_frame_cellb_multi([_lib.FrameCellJob() for _ in range(n)], "st", eps=0.5)
        ops.lucy_tframe_layer_multi(torch.float32, [_lib.TFrameJob() for _ in range(n)], "st",
                                    eps=0.5)
        assert sizes(stub, "sc_lucy_frame_gemm_multi") == want
        assert sizes(stub, "sc_lucy_frame_cellb_multi") == want
        assert sizes(stub, "sc_lucy_tframe_layer_multi") == want
        for name, scalars, jt, _, _, stream in stub.calls:
            assert stream == "st"
            assert (scalars, jt) == {
                "sc_lucy_frame_gemm_multi": ((1, 1, 0.5), _lib.FrameGemmJob),
                "sc_lucy_frame_cellb_multi": ((0.5,), _lib.FrameCellJob),
                "sc_lucy_tframe_layer_multi": ((0, 0.5), _lib.TFrameJob)}[name]


def test_image_and_fold_loops_honour_the_cap(stub):
    w = torch.zeros(2, 4)
    ops._image_jobs([_lib.ImageJob() for _ in range(17)], [w])
    assert sizes(stub, "sc_weight_images") == [16, 1]
    stub.calls.clear()
    ops._image_jobs([], [w])
    assert stub.calls == []
    specs = [(torch.zeros(3, 4), torch.zeros(3), torch.ones(4), torch.zeros(4), 0, 4, False)
             for _ in range(17)]
    out = ops.fold_images(specs)
    assert len(out) == 17 and all(o is not None for o in out)
    assert sizes(stub, "sc_ln_fold_prep") == [16, 1] and sizes(stub, "sc_weight_images") == [16, 1]
    assert {c[2] for c in stub.calls} == {_lib.LnFoldJob, _lib.ImageJob}
    assert all(c[1] == () and c[5] == "stream" for c in stub.calls)
    stub.calls.clear()
    assert ops.fold_images([]) == [] and stub.calls == []
