"""Which kernel a wide-MLP layer gets: ``pmml_gemm_route`` / ``pmml_gemm_fused_head_route`` of
``ops/csrc/gemm.hip`` against a plain-Python twin of the dispatch they replaced.

Every alternative GEMM kernel is pinned bit for bit against the default (``tests/test_wide_mlp.py``,
``tests/test_gpu_exact.py``), so a layer sent to the wrong kernel still computes the right numbers:
only the route itself can show a dispatch slip. ``_twin_launch`` and ``_twin_fused_head`` are
transcribed, statement for statement and with the shifts and literals as they stood, from the
commit before ``route()`` existed (97f6af0: ``pmml_gemm_launch`` + ``launch_k64p`` + ``launch8p`` +
``use8p``, and ``pmml_gemm_fused_head_launch``); they return the name of the kernel that code
launched, 0 where it launched nothing and -4 where it refused. ``KERNELS`` is ``enum GemmKernel``
in order, from id 1.

Nothing is launched: the pointers in the args are made-up, 16-byte-aligned addresses that the
route functions never follow. Such args must never reach a launch entry. The module is marked
``gpu`` because the kernel library is built where the GPU suite runs."""

import ctypes
import itertools

import pytest

pytestmark = pytest.mark.gpu

KERNELS = [
    "gemm_kernel<32,true,true>", "gemm_kernel<256,false,true>", "gemm_kernel<32,true,false>",
    "gemm_kernel<256,false,false,true>", "gemm_kernel<256,false,false>",
    "gemm_k64_kernel<false,true>", "gemm_k64_kernel<false,false>",
    "gemm_k64p_kernel<true,true>", "gemm_k64p_kernel<true>", "gemm_k64p_kernel<false>",
    "gemm8_kernel<false,true>", "gemm8_kernel<false,false>", "gemm8_kernel<true,false>",
    "gemm8p_kernel<false,false>", "gemm8p_kernel<false,true>", "gemm8p_kernel<false,false,true>",
    "gemm8p_kernel<true,false>",
]

# constants of gemm.hip
BM, BK, SLICE_B, HALF_B, P8_SCR = 256, 64, 128, 128 * 128, 8 * 2048
P8_MAX_MP = (160 * 1024 - 8 * HALF_B - P8_SCR) // 4
P8_HEAD_MAX_OUT = P8_SCR // (4 * BM * 4)
P8_HEAD_MAX_MP = (160 * 1024 - 8 * HALF_B - P8_SCR) // (4 + 2 * P8_HEAD_MAX_OUT)
assert (P8_MAX_MP, P8_HEAD_MAX_OUT, P8_HEAD_MAX_MP) == (4096, 4, 1365)

EXPERIMENT_BITS = range(5, 17)
SUBSETS = [sum(1 << b for b, on in zip(EXPERIMENT_BITS, pick) if on)
           for pick in itertools.product((0, 1), repeat=len(EXPERIMENT_BITS))]
PTR = 0x7F0000010000  # a made-up address, 16-byte aligned; every pointer gets its own multiple of 4 KiB


# ----------------------------------------------------------------- the parent's dispatch, in Python

def _use8p(a):
    return (not ((a.flags >> 12) & 1) and a.Mp <= P8_MAX_MP and a.lda * 2 * BM < (1 << 31) and
            a.ldw * 2 * 256 < (1 << 31))


def _twin_launch_k64p(a):
    seg = not ((a.flags >> 10) & 1)
    nts = seg and not ((a.flags >> 14) & 1)
    return "gemm_k64p_kernel<true,true>" if nts else "gemm_k64p_kernel<true>" if seg else "gemm_k64p_kernel<false>"


def _twin_launch8p(a, headf):
    nostore = not headf and ((a.flags >> 13) & 1)
    defer = not headf and not nostore and ((a.flags >> 15) & 1)
    if headf:
        return "gemm8p_kernel<true,false>"
    if nostore:
        return "gemm8p_kernel<false,true>"
    if defer:
        return "gemm8p_kernel<false,false,true>"
    return "gemm8p_kernel<false,false>"


def _twin_launch(a, head):
    if a.rows <= 0:
        return 0
    BN = 32 if head else 256
    if a.flags & ~0x1FFE1:
        return -4
    f32 = a.flags & 1
    ph8 = not f32 and (((a.flags >> 7) & 1) or a.K >= 512)
    sk = SLICE_B // 4 if f32 else SLICE_B // 2
    if a.rows_p % BM or a.rows_p < a.rows or a.K % sk or a.K <= 0 or a.Mp % BN or a.Mp <= 0:
        return -4
    if (a.lda & 7) or (a.ldw & 7) or a.lda < a.K or a.ldw < a.K:
        return -4
    if ((a.A or 0) & 15) or ((a.Wt or 0) & 15):
        return -4
    if head and (a.n_out < 1 or a.n_out > 32 or a.Mp != 32 or
                 (not a.C and (not a.row_ok or not a.score or not a.valid))):
        return -4
    if head and a.C and (a.ldc < a.n_out or (a.C & 3)):
        return -4
    if not head and ((a.ldc & 7) or a.ldc < a.Mp or not a.C or (a.C & 15)):
        return -4
    tst = not ((a.flags >> 8) & 1) and not ((a.flags >> 5) & 1)
    if not head and not f32 and a.K == 64 and not ((a.flags >> 6) & 1):
        if tst and not ((a.flags >> 9) & 1):
            return _twin_launch_k64p(a)
        elif tst:
            return "gemm_k64_kernel<false,true>"
        else:
            return "gemm_k64_kernel<false,false>"
    p8 = (not f32 and tst and not head and not ((a.flags >> 11) & 1) and (a.K >= 128 or ((a.flags >> 7) & 1)) and
          (_use8p(a) or ((a.flags >> 13) & 1) or ((a.flags >> 16) & 1)))
    if f32:
        return "gemm_kernel<32,true,true>" if head else "gemm_kernel<256,false,true>"
    if head:
        return "gemm_kernel<32,true,false>"
    if p8:
        return _twin_launch8p(a, False)
    if ph8:
        return "gemm8_kernel<false,true>" if tst else "gemm8_kernel<false,false>"
    return "gemm_kernel<256,false,false,true>" if tst else "gemm_kernel<256,false,false>"


def _twin_fused_head(a, o, wh_perm=PTR, part=PTR):
    if a.rows <= 0:
        return 0
    if (a.flags & 1) or (o.flags & 1):
        return -4
    if a.rows_p % BM or a.rows_p < a.rows or a.K % BK or a.K <= 0 or a.Mp % 256 or a.Mp <= 0:
        return -4
    if (a.lda & 7) or (a.ldw & 7) or a.lda < a.K or a.ldw < a.K:
        return -4
    if ((a.A or 0) & 15) or ((a.Wt or 0) & 15):
        return -4
    if o.n_out < 1 or o.n_out > 32 or o.K != a.Mp or o.rows != a.rows or o.rows_p != a.rows_p:
        return -4
    if not o.row_ok or not o.score or not o.valid or not part or not wh_perm or (wh_perm & 15):
        return -4
    p8 = _use8p(a) and o.n_out <= P8_HEAD_MAX_OUT and a.Mp <= P8_HEAD_MAX_MP
    return _twin_launch8p(a, True) if p8 else "gemm8_kernel<true,false>"


# ----------------------------------------------------------------- args and the two exports

@pytest.fixture(scope="module")
def lib():
    from flink_jpmml_amd.ops._lib import load

    return load()


def _layer(head=0, f32=0, K=512, Mp=None, lda=None, rows=4000, rows_p=4096, n_out=3):
    """Well-formed args of one layer: a hidden layer writes C; an output layer decodes (C null)."""
    from flink_jpmml_amd.ops._lib import GemmArgs

    a = GemmArgs()
    Mp = Mp if Mp is not None else (32 if head else 256)
    a.A, a.Wt, a.bias = PTR, PTR + 0x1000, PTR + 0x2000
    a.rows, a.rows_p, a.K, a.Mp = rows, rows_p, K, Mp
    a.lda, a.ldw, a.flags = (lda if lda is not None else K), K, f32
    if head:
        a.n_out, a.ldc = n_out, 32
        a.row_ok, a.score, a.valid = PTR + 0x4000, PTR + 0x5000, PTR + 0x6000
    else:
        a.C, a.ldc = PTR + 0x3000, Mp
    return a


def _name(rc):
    return KERNELS[rc - 1] if rc > 0 else rc


def _route(lib, a, head):
    return _name(lib.pmml_gemm_route(ctypes.byref(a), head))


def _fused(lib, a, o):
    return _name(lib.pmml_gemm_fused_head_route(ctypes.byref(a), ctypes.byref(o)))


KS = (32, 64, 128, 192, 448, 512, 1024, 4096)
MPS = (32, 256, 768, 4096, 4352)  # 4096 = P8_MAX_MP: the last width gemm8p_kernel takes; 4352 the first it refuses
LDAS = (None, 4194296, 4194304)   # K, and either side of lda * 2 * BM < 2^31


def _sweep(lib, head, f32, shapes):
    route, twin, seen = lib.pmml_gemm_route, _twin_launch, set()
    for K, Mp in shapes:
        for lda in LDAS:
            a = _layer(head=head, f32=f32, K=K, Mp=Mp, lda=lda)
            ref = ctypes.byref(a)
            for bits in SUBSETS:
                a.flags = bits | f32
                want, got = twin(a, head), route(ref, head)
                assert _name(got) == want, f"head={head} K={K} Mp={Mp} lda={a.lda} flags={a.flags:#x}"
                seen.add(want)
    return seen


def test_bf16_hidden_layers_every_flag_subset(lib):
    seen = _sweep(lib, 0, 0, itertools.product(KS, MPS))
    # the grid reaches every kernel a bf16 hidden layer can get, and the refusals
    assert seen == {-4} | set(KERNELS[3:12]) | set(KERNELS[13:16])


@pytest.mark.parametrize("head,f32", [(0, 1), (1, 0), (1, 1)], ids=["fp32-hidden", "bf16-head", "fp32-head"])
def test_fp32_and_output_layers_every_flag_subset(lib, head, f32):
    seen = _sweep(lib, head, f32, itertools.product(KS, MPS))
    assert seen == {-4, KERNELS[{(0, 1): 1, (1, 0): 2, (1, 1): 0}[head, f32]]}


@pytest.mark.parametrize("head,f32", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_every_shape_without_flags(lib, head, f32):
    for K, Mp, lda in itertools.product(KS, MPS, LDAS):
        a = _layer(head=head, f32=f32, K=K, Mp=Mp, lda=lda)
        assert _route(lib, a, head) == _twin_launch(a, head), f"head={head} f32={f32} K={K} Mp={Mp} lda={a.lda}"


def _set(**fields):
    def change(a):
        for k, v in fields.items():
            setattr(a, k, v)
    return change


REFUSED = [("bit %d" % b, 0, _set(flags=1 << b)) for b in (1, 2, 3, 4, 17)] + [
    ("K not a slice multiple", 0, _set(K=96, lda=96, ldw=96)),
    ("fp32 K not a slice multiple", 0, _set(flags=1, K=48, lda=48, ldw=48)),
    ("rows_p not a multiple of 256", 0, _set(rows_p=4224)),
    ("rows_p < rows", 0, _set(rows=4097)),
    ("lda odd", 0, _set(lda=513)),
    ("ldw odd", 0, _set(ldw=513)),
    ("A at + 8", 0, _set(A=PTR + 8)),
    ("Wt at + 8", 0, _set(Wt=PTR + 0x1008)),
    ("C at + 8", 0, _set(C=PTR + 0x3008)),
    ("hidden with null C", 0, _set(C=None)),
    ("head n_out 0", 1, _set(n_out=0)),
    ("head n_out 33", 1, _set(n_out=33)),
    ("head Mp 64", 1, _set(Mp=64)),
    ("head Mp 256", 1, _set(Mp=256)),
]


@pytest.mark.parametrize("what,head,change", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_args(lib, what, head, change):
    a = _layer(head=head)
    assert _route(lib, a, head) == _twin_launch(a, head) and _twin_launch(a, head) in KERNELS  # taken before the change
    change(a)
    assert _twin_launch(a, head) == -4
    assert _route(lib, a, head) == -4
    a.rows = 0  # nothing to launch comes first, whatever else is wrong
    assert _twin_launch(a, head) == 0
    assert _route(lib, a, head) == 0


def _pair(K=512, Mp=1024, n_out=3, flags=0, **kw):
    a = _layer(K=K, Mp=Mp, **kw)
    a.C, a.ldc, a.flags = None, 0, flags  # the fused hidden layer stores nothing
    o = _layer(head=1, K=Mp, n_out=n_out, **{k: v for k, v in kw.items() if k in ("rows", "rows_p")})
    return a, o


def test_fused_head_every_flag_subset(lib):
    seen = set()
    # P8_HEAD_MAX_OUT = 4; P8_HEAD_MAX_MP = 1365: 1280 is the last multiple of 256 the persistent kernel takes
    for n_out, Mp, lda in itertools.product((4, 5), (1280, 1536), LDAS):
        a, o = _pair(Mp=Mp, n_out=n_out, lda=lda)
        for bits in SUBSETS:
            a.flags = bits
            want = _twin_fused_head(a, o)
            assert _fused(lib, a, o) == want, f"n_out={n_out} Mp={Mp} lda={a.lda} flags={bits:#x}"
            assert (want == "gemm8p_kernel<true,false>") == (
                n_out == 4 and Mp == 1280 and lda != 4194304 and not bits & 0x1000)
            seen.add(want)
    assert seen == {"gemm8p_kernel<true,false>", "gemm8_kernel<true,false>"}


def test_fused_head_refusals(lib):
    a, o = _pair()
    assert _fused(lib, a, o) == _twin_fused_head(a, o) == "gemm8p_kernel<true,false>"
    a.flags = 0x1000  # bit 12: one tile per workgroup
    assert _fused(lib, a, o) == _twin_fused_head(a, o) == "gemm8_kernel<true,false>"
    for change_a, change_o in [(_set(flags=1), _set()), (_set(), _set(flags=1)),      # an fp32 operand
                               (_set(), _set(K=768)),                                # o.K != a.Mp
                               (_set(), _set(n_out=0)), (_set(), _set(n_out=33)),
                               (_set(), _set(rows=3999)), (_set(), _set(rows_p=4352)),
                               (_set(), _set(score=None)), (_set(), _set(row_ok=None)), (_set(), _set(valid=None)),
                               (_set(K=96, lda=96, ldw=96), _set()), (_set(A=PTR + 8), _set()),
                               (_set(Wt=PTR + 0x1008), _set()), (_set(lda=513), _set())]:
        a, o = _pair()
        change_a(a), change_o(o)
        assert _twin_fused_head(a, o) == -4
        assert _fused(lib, a, o) == -4
        a.rows = 0
        assert _fused(lib, a, o) == _twin_fused_head(a, o) == 0
