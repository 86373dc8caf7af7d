"""Case table of tests/test_gpu_gemm_paths.py: one row per dispatch path of gemm_auto -> launch_gemm (csrc/gemm.hip) for plain operand pairs, the rows of
nmfx_gemm64 and the counts of the two device helpers.  Imports without a GPU; tests/test_gemm_paths_host.py keeps the table honest on the CPU.

A row names the path it is meant to reach (`expect`); classify() restates the host-side dispatch rules (gemm_tile_shape, pipe_ok, launch_gemm, gemm_pick_split,
tiny_size, tiny_split, reduce_slabs) so that a row whose shape stops reaching its path is noticed without a GPU.  The restatement is checked against the kernels a
run really launches by a kernel trace of the GPU file, not by these tests.

Storage (column-major, as the C ABI takes it): op 0 stores A as M x Kc and B as Kc x N, op 1 stores the transposes.  A leading dimension is "stored rows + pad";
`off` shifts a base pointer by that many elements inside a larger allocation.  Every element outside the matrices is NaN (operands) or a sentinel NaN (C)."""
import zlib

import numpy as np

U24, U53 = 2.0 ** -24, 2.0 ** -53
BK = 32
TRAIL = 64                                    # sentinel elements kept behind every output
SENT32, SENT64 = 0x7FC0BEEF, 0x7FF8DEADBEEF0001
PRO_NAMES = {0: "none", 1: "ratio", 2: "ratio_sq", 3: "recip2", 4: "diff", 5: "powprod"}
OPS = ((0, 0), (0, 1), (1, 0), (1, 1))

# the project's norm bounds (tests/test_gpu_kernels.py)
NORM_UNSPLIT, NORM_SPLIT = 2e-6, 3e-6
NORM_C64, NORM_C32 = 1e-14, 1e-7


# ---- the table ----------------------------------------------------------------------------------------------------------------------------------------
CASES = {}


def _add(name, shape, ops, expect, pad=(0, 0, 0), off=(0, 0), proA=0, proB=0, acc=0, ws=True, per_element_only=False):
    assert name not in CASES, name
    CASES[name] = dict(name=name, shape=shape, ops=ops, pad=pad, off=off, proA=proA, proB=proB, acc=acc, ws=ws, expect=expect, per_element_only=per_element_only)


def _opname(ops):
    return "%s%s" % ("nt"[ops[0]], "nt"[ops[1]])


WHOLE_SPLIT = dict(path="whole", tile=(128, 128), split=5, reduce="plain")
WHOLE_REMAP = dict(path="whole", tile=(128, 128), split=1, remap=True)
EDGE_VEC = dict(path="edge_vec", tile=(128, 128), split=1, remap=True)
EDGE_DWORD = dict(path="edge_dword", tile=(128, 128), split=1)
EDGE_SHORTK = dict(path="edge_vec", tile=(128, 128), split=2, reduce="plain")
EDGE_LANES = dict(path="edge_vec", tile=(128, 128), split=26, reduce="lanes")
EDGE_LANES_COL = dict(path="edge_vec", tile=(128, 128), split=26, reduce="lanes_percol")
EDGE_NOWS = dict(path="edge_vec", tile=(128, 128), split=1)
LANES_COL = dict(path="edge_vec", tile=(128, 128), split=250, reduce="lanes_percol")
TINY = dict(path="tiny", split=1)
TINY_SPLIT = dict(path="tiny", split=64, reduce="lanes")
HEAVY_FAST = dict(path="heavy_fast", split=1)
HEAVY_GUARD = dict(path="heavy_guard", split=1)

for ops in OPS:
    _add("whole_split_" + _opname(ops), (128, 256, 672), ops, WHOLE_SPLIT)
for pro in (1, 2, 3, 4):
    for ops in ((0, 0), (1, 1)):
        _add("whole_split_%s_A_%s" % (PRO_NAMES[pro], _opname(ops)), (128, 256, 672), ops, WHOLE_SPLIT, proA=pro)
        _add("whole_split_%s_B_%s" % (PRO_NAMES[pro], _opname(ops)), (128, 256, 672), ops, WHOLE_SPLIT, proB=pro)
for ops in ((0, 0), (1, 1)):
    _add("whole_remap_" + _opname(ops), (2048, 2048, 32), ops, WHOLE_REMAP)
for ops in OPS:
    _add("edge_vec_" + _opname(ops), (500, 508, 72), ops, EDGE_VEC)
    _add("edge_vec_padded_acc_" + _opname(ops), (500, 508, 72), ops, EDGE_VEC, pad=(4, 4, 4), acc=1)
    _add("edge_dword_odd_" + _opname(ops), (501, 510, 70), ops, EDGE_DWORD)
    _add("edge_dword_lda_" + _opname(ops), (500, 508, 72), ops, EDGE_DWORD, pad=(1, 0, 0))
    _add("edge_dword_ldb_" + _opname(ops), (500, 508, 72), ops, EDGE_DWORD, pad=(0, 1, 0))
    _add("edge_dword_ptrA_" + _opname(ops), (500, 508, 72), ops, EDGE_DWORD, pad=(4, 4, 0), off=(1, 0))
    _add("edge_dword_ptrB_" + _opname(ops), (500, 508, 72), ops, EDGE_DWORD, pad=(4, 4, 0), off=(0, 1))
    _add("edge_shortk_split_" + _opname(ops), (256, 256, 264), ops, EDGE_SHORTK)
for acc in (0, 1):
    _add("edge_lanes_acc%d" % acc, (132, 132, 4100), (0, 0), EDGE_LANES, acc=acc)
    _add("edge_lanes_ldc_acc%d" % acc, (132, 132, 4100), (0, 0), EDGE_LANES_COL, pad=(0, 0, 4), acc=acc)
    _add("edge_nows_acc%d" % acc, (132, 132, 4100), (0, 0), EDGE_NOWS, acc=acc, ws=False, per_element_only=True)
    _add("lanes_percol_acc%d" % acc, (36, 20, 40000), (0, 0), LANES_COL, pad=(0, 0, 4), acc=acc)
for pro in (1, 2, 3, 4):
    for ops in ((0, 0), (1, 1)):
        for shape, tag, exp in (((260, 132, 500), "vec", dict(path="edge_vec", tile=(128, 128), split=4, reduce="plain")),
                                ((257, 131, 501), "dword", dict(path="edge_dword", tile=(128, 128), split=4, reduce="plain"))):
            _add("edge_%s_%s_A_%s" % (tag, PRO_NAMES[pro], _opname(ops)), shape, ops, exp, proA=pro, acc=1)
            _add("edge_%s_%s_B_%s" % (tag, PRO_NAMES[pro], _opname(ops)), shape, ops, exp, proB=pro, acc=1)
for ops in OPS:
    _add("tiny_ldc_" + _opname(ops), (100, 37, 53), ops, TINY, pad=(0, 0, 4))
    _add("tiny_split64_" + _opname(ops), (5, 5, 100000), ops, TINY_SPLIT)
    _add("tiny_long_ldc_" + _opname(ops), (5, 5, 100000), ops, TINY, pad=(0, 0, 3))
for ops in ((0, 0), (1, 1)):
    for shape, tag, exp in (((128, 128, 64), "aligned", HEAVY_FAST), ((130, 70, 100), "ragged", HEAVY_GUARD)):
        _add("powprod_%s_A_%s" % (tag, _opname(ops)), shape, ops, exp, proA=5)
        _add("powprod_%s_B_%s" % (tag, _opname(ops)), shape, ops, exp, proB=5)

NAMES = list(CASES)


# ---- the dispatch rules of csrc/gemm.hip and aux.hip::reduce_slabs, restated ----------------------------------------------------------------------------------
def stored_shape(c, which):
    """(rows, cols) of operand `which` ('A' or 'B') as it lies in memory"""
    M, N, Kc = c["shape"]
    if which == "A":
        return (M, Kc) if c["ops"][0] == 0 else (Kc, M)
    return (Kc, N) if c["ops"][1] == 0 else (N, Kc)


def leading_dims(c):
    return stored_shape(c, "A")[0] + c["pad"][0], stored_shape(c, "B")[0] + c["pad"][1], c["shape"][0] + c["pad"][2]


def tile_shape(M, N):
    bm, bn = 128, 128
    if M % 128 != 0 and M % 64 == 0:
        bm = 64
    if bm == 128 and N % 128 != 0 and N % 64 == 0 and N <= 192:
        bn = 64
    if bm == 128 and bn == 128 and M % 128 == 0 and N % 128 == 0 and (M // 128) * (N // 128) < 256 and M >= 256:
        bm = 64
    return bm, bn


def pick_split(M, N, Kc):
    bm, bn = tile_shape(M, N)
    tiles = -(-M // bm) * -(-N // bn)
    ktiles = -(-Kc // BK)
    split = 1
    if tiles < 512 and ktiles >= 8:
        split = min(-(-512 // tiles), 256)
        split = min(split, ktiles // 4)
    return max(split, 1)


def tiny_size(M, N, Kc):
    return 2 * M * N * Kc <= 1 << 25


def tiny_split(M, N, Kc):
    if Kc >= 256 and M * N <= 65536:
        per = max(32, (Kc + 63) // 64)
        return -(-Kc // per), per
    return 1, Kc


def _reduce_kind(nslab, count):
    return "lanes" if nslab >= 16 and count <= 1 << 18 else "plain"


def classify(c):
    """the path nmfx_gemm_f32 takes for row c (base allocations are 16-byte aligned, the workspace holds every slab)"""
    M, N, Kc = c["shape"]
    a_kc, b_kc = c["ops"][0] == 1, c["ops"][1] == 0
    lda, ldb, ldc = leading_dims(c)
    pro = c["proA"] != 0 or c["proB"] != 0
    heavy = 5 in (c["proA"], c["proB"])
    out = dict(a_kc=a_kc, b_kc=b_kc, pro=pro)
    if not c["acc"] and not pro and tiny_size(M, N, Kc):
        S, per = tiny_split(M, N, Kc) if (ldc == M and c["ws"]) else (1, Kc)
        out.update(path="tiny", split=S, per=per)
        if S > 1:
            out["reduce"] = _reduce_kind(S, M * N)
        return out
    split, kspan = 1, Kc
    if c["ws"]:
        split = pick_split(M, N, Kc)
    if split > 1:
        kspan = -(-(-(-Kc // BK)) // split) * BK
        split = -(-Kc // kspan)
    views = lda % 4 == 0 and ldb % 4 == 0 and c["off"][0] % 4 == 0 and c["off"][1] % 4 == 0
    tm, tn = tile_shape(M, N)
    fast = M % tm == 0 and N % tn == 0 and Kc % BK == 0 and kspan % BK == 0 and views
    vec = views and (Kc % 4 == 0 if a_kc else M % 4 == 0) and (Kc % 4 == 0 if b_kc else N % 4 == 0)
    bm, bn = (tm, tn) if fast and not heavy else (128, 128)
    if heavy:
        out.update(path="heavy_fast" if fast and M % 128 == 0 and N % 128 == 0 else "heavy_guard")
    elif vec and fast:      # launch_gemm's `whole` for plain views
        out.update(path="whole")
    else:
        out.update(path="edge_vec" if vec else "edge_dword")
    grid = -(-M // bm) * -(-N // bn)
    out.update(tile=(bm, bn), split=split, per=kspan, remap=(not heavy and grid % 8 == 0 and grid >= 16))
    if split > 1:
        out["reduce"] = _reduce_kind(split, M if ldc != M else M * N) + ("_percol" if ldc != M else "")
    return out


def kernel_signature(c):
    """the template arguments of the product kernel row c launches, as a kernel trace prints them"""
    k = classify(c)
    b = lambda x: "true" if x else "false"
    if k["path"] == "tiny":
        return "tiny_gemm_kernel"
    if k["path"].startswith("heavy"):
        return "gemm_kernel<128, 128, %s, %s, %s, true>" % (b(k["a_kc"]), b(k["b_kc"]), b(k["path"] == "heavy_fast"))
    return "gemm_pipe_kernel<%d, %d, %s, %s, %s, %s, %s>" % (k["tile"] + (b(k["a_kc"]), b(k["b_kc"]), b(k["pro"]), b(k["path"] != "edge_dword"), b(k["path"] != "whole")))


# ---- inputs, reference and bounds ----------------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _mapped(pro, X, X2):
    if pro == 0:
        return X
    return {1: X / X2, 2: X / X2 ** 2, 3: 1.0 / X2, 4: X2 - X, 5: np.ones_like(X)}[pro]


_BUILT = {}


def build(name):
    """inputs of row `name` in their LOGICAL shapes op(A): M x Kc, op(B): Kc x N (fp32 values held as float64), the float64 reference and the bounds.  Cached and
    never modified by the tests."""
    if name in _BUILT:
        return _BUILT[name]
    c = CASES[name]
    M, N, Kc = c["shape"]
    rs = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    A, B = _f32(rs.rand(M, Kc) - 0.3), _f32(rs.rand(Kc, N) - 0.3)
    A2 = _f32(rs.rand(M, Kc) + 0.1) if c["proA"] else None
    B2 = _f32(rs.rand(Kc, N) + 0.1) if c["proB"] else None
    C0 = _f32(rs.rand(M, N)) if c["acc"] else None
    fA, fB = _mapped(c["proA"], A, A2), _mapped(c["proB"], B, B2)
    ref = fA @ fB + (C0 if c["acc"] else 0.0)
    absprod = np.abs(fA) @ np.abs(fB)
    tiny = c["expect"]["path"] == "tiny"
    # fp32 dot product of Kc terms in any order + the 1-ulp v_rcp_f32 of the maps + the final rounding(s): (Kc + 8) u |op(A)| |op(B)|; with `accumulate` the
    # rounding of the closing add is u (|product| + |C0|) <= 2 u |op(A)| |op(B)| as long as |C0| <= |op(A)| |op(B)| (asserted by the host test), inside the + 8.
    # tiny: fp64 accumulation, one rounding of the result
    bound = U24 * np.abs(ref) + Kc * U53 * absprod if tiny else (Kc + 8) * U24 * absprod
    norm = None if c["per_element_only"] else (NORM_SPLIT if c["expect"]["split"] > 1 else NORM_UNSPLIT)
    for x in (A, B, A2, B2, C0, ref, absprod, bound):
        if x is not None:
            x.setflags(write=False)
    _BUILT[name] = dict(A=A, B=B, A2=A2, B2=B2, C0=C0, ref=ref, absprod=absprod, bound=bound, norm=norm)
    return _BUILT[name]


def stored(c, which, X):
    """logical op(X) -> the matrix as stored"""
    op = c["ops"][0 if which == "A" else 1]
    return X if op == 0 else X.T


def pack(X, ld, off, dtype=np.float32, tail=0):
    """column-major image of X (rows x cols) with leading dimension ld behind `off` elements; everything that is not an element of X is NaN"""
    rows, cols = X.shape
    assert ld >= rows
    buf = np.full(off + ld * cols + tail, np.nan, dtype=dtype)
    buf[off:off + ld * cols].reshape(cols, ld)[:, :rows] = X.T
    return buf


def sentinel(count, dtype=np.float32):
    return np.full(count, SENT32 if dtype == np.float32 else SENT64, dtype=np.uint32 if dtype == np.float32 else np.uint64).view(dtype)


def pack_c(C0, M, N, ldc, dtype=np.float32):
    """the output buffer: ldc * N elements + TRAIL behind them, all sentinel NaN but for C0 (when given)"""
    buf = sentinel(ldc * N + TRAIL, dtype)
    if C0 is not None:
        buf[:ldc * N].reshape(N, ldc)[:, :M] = C0.T
    return buf


def unpack_c(buf, M, N, ldc):
    """-> (C as M x N, True where an element is NOT part of C)"""
    inside = np.zeros(buf.shape, dtype=bool)
    inside[:ldc * N].reshape(N, ldc)[:, :M] = True
    return buf[:ldc * N].reshape(N, ldc)[:, :M].T, ~inside


def judge(buf, buf2, M, N, ldc, ref, bound, norm):
    """What every product is held to, on the whole output buffer of two calls: -> (figures, list of what is wrong).  Shared by the GPU test and by the host test
    that plants defects, so that the checks themselves are tested."""
    bits = np.uint32 if buf.dtype == np.float32 else np.uint64
    got, outside = unpack_c(buf, M, N, ldc)
    sent = sentinel(buf.size, buf.dtype.type).view(bits)
    finite = bool(np.all(np.isfinite(got)))
    err = np.abs(got.astype(np.float64) - ref)
    q = np.nan_to_num(err / bound, nan=np.inf)
    worst = tuple(int(x) for x in np.unravel_index(int(np.argmax(q)), q.shape))
    fig = dict(ratio=float(q.max()), worst=worst, rel_fro=float(np.linalg.norm(err) / np.linalg.norm(ref)) if finite else float("inf"))
    wrong = []
    if not np.array_equal(buf.view(bits)[outside], sent[outside]):
        wrong.append("padding or trailing elements of C were written")
    if not finite:
        wrong.append("NaN / Inf in C: padding of an operand or of C reached the product")
    if not fig["ratio"] <= 1.0:
        wrong.append("per-element bound exceeded %.3f times at %s" % (fig["ratio"], worst))
    if norm is not None and not fig["rel_fro"] < norm:
        wrong.append("rel_fro %.3e >= %g" % (fig["rel_fro"], norm))
    if not np.array_equal(buf.view(bits), buf2.view(bits)):
        wrong.append("two calls on the same inputs differ")
    return fig, wrong


# ---- nmfx_gemm64 -------------------------------------------------------------------------------------------------------------------------------------
G64_CASES = {}
for _name, _shape, _pad, _kern, _types in (("panel2_ragged", (2100, 930, 64), (0, 0, 0), "panel<2,8,1,2>", ((True, False),)),
                                           ("panel1_padded", (1000, 130, 256), (4, 4, 2), "panel<1,8,1,2>", ((True, False),)),
                                           ("tiled_padded", (300, 77, 112), (4, 4, 2), "tiled", ((True, False), (False, False), (True, True), (False, True)))):
    for _a64, _b64 in _types:
        for _outs in ("both", "c64", "c32"):
            _n = "%s_%s%s_%s" % (_name, "d" if _a64 else "s", "d" if _b64 else "s", _outs)
            G64_CASES[_n] = dict(name=_n, shape=_shape, pad=_pad, kernel=_kern, a64=_a64, b64=_b64, outs=_outs)
G64_NAMES = list(G64_CASES)


def g64_kernel(c):
    """gemm64.hip::gemm64's choice, restated"""
    M, N, Kc = c["shape"]
    if c["a64"] and not c["b64"] and Kc % 32 == 0 and Kc <= 512 and M >= 256:
        return "panel<2,8,1,2>" if -(-M // 256) * -(-N // 32) >= 256 else "panel<1,8,1,2>"
    return "tiled"


def _exact_product(A, B):
    """A @ B with an extended-precision accumulator where the platform has one (x86: 64-bit mantissa), so that the reference carries none of the float64 chain's
    own rounding; plain float64 otherwise"""
    if np.finfo(np.longdouble).eps < 2.0 ** -60:
        return (A.astype(np.longdouble) @ B.astype(np.longdouble)).astype(np.float64)
    return A @ B


_G64_BUILT = {}


def g64_build(name):
    c = G64_CASES[name]
    key = (c["shape"], c["a64"], c["b64"])
    if key in _G64_BUILT:
        return _G64_BUILT[key]
    M, N, Kc = c["shape"]
    rs = np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)
    A, B = rs.rand(M, Kc) - 0.3, rs.rand(Kc, N) - 0.3
    if not c["a64"]:
        A = _f32(A)
    if not c["b64"]:
        B = _f32(B)
    ref = _exact_product(A, B)
    absprod = np.abs(A) @ np.abs(B)
    b64 = Kc * U53 * absprod
    b32 = b64 + U24 * np.abs(ref)
    for x in (A, B, ref, absprod, b64, b32):
        x.setflags(write=False)
    _G64_BUILT[key] = dict(A=A, B=B, ref=ref, absprod=absprod, bound64=b64, bound32=b32)
    return _G64_BUILT[key]


# ---- device helpers -------------------------------------------------------------------------------------------------------------------------------------
HELPER_COUNTS = (1, 63, 256, 257, 1024 * 256 + 777)      # the last: longer than one pass of the 1024 x 256 grid
PLACEMENTS = ("first", "last", "tail")
SCALE_DIVIDE_BY = 3.7


def minmax_input(count, placement, negative):
    """fp32 data with its maximum and its minimum planted: 'first' max at 0 / min at the end, 'last' the other way round, 'tail' both behind the last multiple of 256"""
    rs = np.random.RandomState(count % 100003 + 7 * PLACEMENTS.index(placement) + (1 if negative else 0))
    X = (rs.rand(count) + (-0.5 if negative else 0.5)).astype(np.float32)
    hi, lo = np.float32(7.25), np.float32(-9.5 if negative else 0.125)
    t0 = 256 * ((count - 1) // 256)
    pmax, pmin = {"first": (0, count - 1), "last": (count - 1, 0), "tail": (t0, count - 1 if count - 1 > t0 else t0 - 1)}[placement]
    if count > 1:
        X[pmin] = lo      # (a one-element tail: the minimum goes right in front of it)
    X[pmax] = hi
    return X


def scale_input(count):
    """values whose quotient by SCALE_DIVIDE_BY stays in fp32's normal range, of both signs, with exact zeros"""
    rs = np.random.RandomState(count % 100003)
    X = ((rs.rand(count) - 0.3) * 10.0 ** rs.randint(-6, 7, size=count)).astype(np.float32)
    X[::5] = 0.0
    if count > 2:
        X[-1] = np.float32(123.456)
    return X


def scale_reference(X):
    return (X.astype(np.float64) / SCALE_DIVIDE_BY).astype(np.float32)
