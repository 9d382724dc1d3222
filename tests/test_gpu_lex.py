"""GPU: rsx_lexsort_device / rsx_sort_columns_device (radix_lexsort, radix_sort_columns) against tests/lex_ref.py.

Every array sits in an allocation the test owns (segment_pairs_gpu.guarded): 64 guard bytes of 0xA5, the array (outputs
filled with 0xA5), 64 guard bytes.  What comes back is compared whole, as bytes: the outputs with the reference's bytes
inside the same guards, the inputs of radix_lexsort with what was put in.  All comparisons are exact.

The matrix.  Column sets: the eight whose plans tests/test_lex_host.py pins -- one round with compound keys of 2, 4, 8
and 16 bytes, with and without pad bytes, sixteen columns in one key, two rounds, three rounds -- and a single f32
column.  Sizes: 1, 2; 256 * VEC - 1, 256 * VEC and 256 * VEC + 1 for the VEC (elements per thread of the join kernel:
2 for 8-byte elements, else 1) of every round of the set: the element-by-element tail and the edge of a workgroup;
20011, past the one-workgroup sort of every element size; and, for (i32,f32), (i64,i64,i32) and (u128,u128,f32),
2^20 + 3, a sort that goes through memory.  Directions: all ascending, all descending, alternating from descending.
Data, both forms in every case: (i) every column from 3 to 5 values of its type -- floats from the special patterns of
test_gpu_unique.py, so that -0.0 / +0.0 and both NaNs occur -- whence rows tie in every column and stability decides;
(ii) any bits.  Nothing is thinned: every set runs every size with every direction pattern in both forms; the index type
alternates int32 / int64 with the parity of (size index + form index), and both are checked on one input in a test of
their own."""
import numpy as np
import pytest

import util
from lex_ref import columns_reference, lex_reference
from pairs_ref import pairs_reference
from segment_pairs_gpu import guarded, same
from segment_pairs_ref import with_guards
from test_gpu_unique import F32_SPECIALS, F64_SPECIALS

pytestmark = pytest.mark.gpu

COLUMN_SETS = {
    "u8,u8": ["u8", "u8"],
    "u16,u8": ["u16", "u8"],
    "i32,f32": ["i32", "f32"],
    "i64,i32": ["i64", "i32"],
    "f64,i64": ["f64", "i64"],
    "16xu8": ["u8"] * 16,
    "i64,i64,i32": ["i64", "i64", "i32"],
    "u128,u128,f32": ["u128", "u128", "f32"],
    "f32": ["f32"],
}
# RSX_INFO_LAST_LEX of each set: (rounds, element bytes of the last round), and the element bytes of every round
INFO = {"u8,u8": (1, 8), "u16,u8": (1, 8), "i32,f32": (1, 16), "i64,i32": (1, 32), "f64,i64": (1, 32), "16xu8": (1, 32),
        "i64,i64,i32": (2, 16), "u128,u128,f32": (3, 32), "f32": (1, 8)}
ROUND_ELEMS = {"u8,u8": [8], "u16,u8": [8], "i32,f32": [16], "i64,i32": [32], "f64,i64": [32], "16xu8": [32],
               "i64,i64,i32": [32, 16], "u128,u128,f32": [8, 32, 32], "f32": [8]}
BIG_SETS = ["i32,f32", "i64,i64,i32", "u128,u128,f32"]
PATTERNS = ["asc", "desc", "alt"]
BIG = 2 ** 20 + 3


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def rs():
    import radix_sort_amd as rs
    return rs


@pytest.fixture(scope="module")
def ctx(rs, torch):
    return rs.Context(torch.cuda.current_device())


# ---- inputs ----
def specs_of(names):
    return [(util.TYPES[t][2], util.TYPES[t][3]) for t in names]


def directions(pattern, m):
    return {"asc": [False] * m, "desc": [True] * m, "alt": [j % 2 == 0 for j in range(m)]}[pattern]


def sizes_of(name):
    ns = {1, 2, 20011}
    for es in ROUND_ELEMS[name]:
        vec = 2 if es == 8 else 1
        ns |= {256 * vec - 1, 256 * vec, 256 * vec + 1}
    return sorted(ns)


def draw(rng, n, tname, form):
    """(n, kb) uint8 raw keys of one column: form 0 from 3 .. 5 values of the type, form 1 any bits."""
    _es, _ko, kb, kind = util.TYPES[tname]
    if form == 1:
        return rng.integers(0, 256, size=(n, kb), dtype=np.uint8)
    k = int(rng.integers(3, 6))
    if kind == util.FLOAT:
        sp = (F32_SPECIALS if kb == 4 else F64_SPECIALS).view(np.uint8).reshape(7, kb)
        pool = sp[rng.choice(7, size=k, replace=False)]
        if k == 3:  # -0.0 and +0.0 always meet
            pool = sp[[2, 3, int(rng.choice([0, 1, 4, 5, 6]))]]
    else:
        pool = rng.integers(0, 256, size=(k, kb), dtype=np.uint8)
        pool[0, -1] |= 0x80  # both signs
        pool[1, -1] &= 0x7F
    return np.ascontiguousarray(pool[rng.integers(0, k, size=n)])


def make_columns(names, n, form, seed):
    rng = np.random.default_rng(seed)
    return [draw(rng, n, t, form) for t in names]


def torch_dtype(torch, tname):
    return {"u8": torch.uint8, "i8": torch.int8, "u16": torch.uint16, "i16": torch.int16, "u32": torch.uint32, "i32": torch.int32,
            "u64": torch.uint64, "i64": torch.int64, "f32": torch.float32, "f64": torch.float64}[tname]


def column_tensor(torch, mid, tname):
    """The column the library is given: a typed view of the guarded bytes; 128-bit keys as (n, 16) bytes."""
    if util.TYPES[tname][2] == 16:
        t = mid.view(-1, 16)
        return (t, util.TYPES[tname][3]) if util.TYPES[tname][3] else t
    return mid.view(torch_dtype(torch, tname))


def upload(torch, names, cols):
    bufs = [guarded(torch, c) for c in cols]
    return bufs, [column_tensor(torch, mid, t) for (_buf, mid), t in zip(bufs, names)]


def index_bytes(perm, idt_bytes):
    return perm.astype("<i4" if idt_bytes == 4 else "<i8").view(np.uint8)


def run_lexsort(rs, torch, c, names, cols, desc, ib, what):
    """radix_lexsort on guarded copies into a guarded index of 0xA5 bytes; inputs and guards checked -> index allocation"""
    n = cols[0].shape[0]
    bufs, tensors = upload(torch, names, cols)
    ibuf, imid = guarded(torch, np.full(n * ib, 0xA5, dtype=np.uint8))
    out = imid.view(torch.int32 if ib == 4 else torch.int64)
    got = rs.radix_lexsort(tensors, descending=desc, out=out, ctx=c)
    assert got is out
    c.check()
    for j, (buf, _mid) in enumerate(bufs):
        assert same(buf.cpu().numpy(), with_guards(cols[j]), ("radix_lexsort changed column", j, what))
    return ibuf.cpu().numpy()


def check_lexsort(rs, torch, c, name, n, pattern, form, ib):
    names = COLUMN_SETS[name]
    desc = directions(pattern, len(names))
    cols = make_columns(names, n, form, seed=n * 31 + form * 7 + PATTERNS.index(pattern))
    want = lex_reference(cols, specs_of(names), desc)
    got = run_lexsort(rs, torch, c, names, cols, desc, ib, (name, n, pattern, form))
    assert same(got, with_guards(index_bytes(want, ib)), ("index", name, n, pattern, form, ib))
    if n >= 2:
        rounds, es = INFO[name]
        assert c.get_info(rs.INFO_LAST_LEX) == rounds | es << 8, (name, n, hex(c.get_info(rs.INFO_LAST_LEX)))


# ---- the matrix ----
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", list(COLUMN_SETS))
def test_lexsort_matrix(rs, torch, ctx, name, pattern):
    for si, n in enumerate(sizes_of(name)):
        for form in (0, 1):
            check_lexsort(rs, torch, ctx, name, n, pattern, form, 4 if (si + form) % 2 == 0 else 8)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", BIG_SETS)
def test_lexsort_through_memory(rs, torch, ctx, name, pattern, form):
    check_lexsort(rs, torch, ctx, name, BIG, pattern, form, 4 if form == 0 else 8)


def test_rounds_are_reported(rs, torch, ctx):
    """One, two and three rounds, and the element of the last one: a silent one-round shortcut would not report them."""
    seen = set()
    for name in COLUMN_SETS:
        check_lexsort(rs, torch, ctx, name, 1000, "alt", 0, 8)
        info = ctx.get_info(rs.INFO_LAST_LEX)
        assert (info & 0xFF, info >> 8 & 0xFF) == INFO[name] and info >> 16 == 0, (name, hex(info))
        assert info & 0xFF == len(rs.lex_plan(specs_of(COLUMN_SETS[name])))
        seen.add(info & 0xFF)
    assert seen == {1, 2, 3}


def test_index_types_and_the_default(rs, torch, ctx):
    names = COLUMN_SETS["i64,i64,i32"]
    n = 20011
    cols = make_columns(names, n, 0, seed=5)
    desc = [False, True, False]
    want = lex_reference(cols, specs_of(names), desc)
    for ib in (4, 8):
        got = run_lexsort(rs, torch, ctx, names, cols, desc, ib, "index types")
        assert same(got, with_guards(index_bytes(want, ib)), ("index", ib))
    _bufs, tensors = upload(torch, names, cols)
    p = rs.radix_lexsort(tensors, descending=desc, ctx=ctx)
    ctx.check()
    assert p.dtype == torch.int64 and p.shape == (n,) and np.array_equal(p.cpu().numpy(), want)
    # a bool for every column, and the default context
    p = rs.radix_lexsort(tensors, descending=True)
    rs.default_context(torch.cuda.current_device()).check()
    assert np.array_equal(p.cpu().numpy(), lex_reference(cols, specs_of(names), [True] * 3))
    # no rows
    empty = [t[:0] for t in tensors]
    assert rs.radix_lexsort(empty, ctx=ctx).shape == (0,)
    ibuf, imid = guarded(torch, np.zeros(0, dtype=np.uint8))
    ctx.lexsort_device([(tensors[0].data_ptr(), 8, 1, False)], ibuf.data_ptr() + 64, 0, 8, torch.cuda.current_stream().cuda_stream)
    ctx.check()
    assert same(ibuf.cpu().numpy(), with_guards(np.zeros(0, dtype=np.uint8)), "n == 0 wrote")


@pytest.mark.parametrize("tname", ["f32", "i64", "u128", "u8"])
def test_one_column_is_radix_argsort(rs, torch, ctx, tname):
    for n, form in ((513, 0), (20011, 0), (20011, 1)):
        cols = make_columns([tname], n, form, seed=n + form)
        for desc in (False, True):
            for idt, ib in ((torch.int32, 4), (torch.int64, 8)):
                got = run_lexsort(rs, torch, ctx, [tname], cols, [desc], ib, ("one column", tname))
                _buf, mid = guarded(torch, cols[0])
                t = column_tensor(torch, mid, tname)
                ibuf, imid = guarded(torch, np.full(n * ib, 0xA5, dtype=np.uint8))
                rs.radix_argsort(t, descending=desc, out=imid.view(idt), ctx=ctx)
                ctx.check()
                assert same(got, ibuf.cpu().numpy(), ("radix_argsort", tname, n, form, desc, ib))


def test_two_u32_columns_are_one_u64_key(rs, torch, ctx):
    """Independent of lex_ref: (a, b) orders as the 64-bit integer a << 32 | b, and (a descending, b) as ~a << 32 | b."""
    rng = np.random.default_rng(21)
    for n in (511, 20011, 300007):
        a = rng.integers(0, 7, size=n, dtype=np.uint32) * np.uint32(0x24924925)  # few values: b decides, then stability
        b = rng.integers(0, 2 ** 32, size=n, dtype=np.uint32)
        b[rng.random(n) < 0.5] = np.uint32(0xFFFFFFFF)
        ta = torch.from_numpy(a.view(np.int32).copy()).cuda().view(torch.uint32)
        tb = torch.from_numpy(b.view(np.int32).copy()).cuda().view(torch.uint32)
        for desc, top in (([False, False], a), ([True, False], ~a)):
            packed = (top.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)
            tp = torch.from_numpy(packed.view(np.int64).copy()).cuda().view(torch.uint64)
            want = rs.radix_argsort(tp, ctx=ctx)
            got = rs.radix_lexsort([ta, tb], descending=desc, ctx=ctx)
            ctx.check()
            assert torch.equal(got, want), (n, desc)
            assert np.array_equal(got.cpu().numpy(), np.argsort(packed, kind="stable"))


def test_a_misaligned_column(rs, torch, ctx):
    """b = base[1:] of an int16 tensor is 2-byte but not 4-byte aligned: the join takes that column key by key."""
    n = 4099
    rng = np.random.default_rng(9)
    a = rng.integers(-3, 3, size=n, dtype=np.int16)
    base = rng.integers(-40, 40, size=n + 1, dtype=np.int16)
    ta = torch.from_numpy(a.copy()).cuda()
    tbase = torch.from_numpy(base.copy()).cuda()
    tb = tbase[1:]
    assert tb.data_ptr() % 4 == 2 and tb.is_contiguous()
    fresh = tb.clone()
    assert fresh.data_ptr() % 16 == 0
    want = lex_reference([a, base[1:]], [(2, util.SIGNED)] * 2, [False, True])
    for cols in ([ta, tb], [tb, ta]):
        got = rs.radix_lexsort(cols, descending=[False, True], ctx=ctx)
        aligned = rs.radix_lexsort([fresh if t is tb else t for t in cols], descending=[False, True], ctx=ctx)
        ctx.check()
        assert torch.equal(got, aligned)
        if cols[0] is ta:
            assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(tbase.cpu().numpy(), base)
    # the same column sorted in place: its neighbour base[0] stays
    va = ta.clone()
    rs.radix_sort_columns([va, tb], descending=[False, True], ctx=ctx)
    ctx.check()
    out = tbase.cpu().numpy()
    assert out[0] == base[0] and np.array_equal(out[1:], base[1:][want]) and np.array_equal(va.cpu().numpy(), a[want])


# ---- radix_sort_columns ----
def run_sort_columns(rs, torch, c, names, cols, desc, values, what):
    """radix_sort_columns on guarded copies -> the whole allocations of the columns and of the values (None without)"""
    n = cols[0].shape[0]
    bufs, tensors = upload(torch, names, cols)
    vbuf = vt = None
    if values is not None:
        vbuf, vmid = guarded(torch, values)
        vt = vmid.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[values.dtype.itemsize]).view((n,) + values.shape[1:])
    assert rs.radix_sort_columns(tensors, values=vt, descending=desc, ctx=c) is None
    c.check()
    return [b.cpu().numpy() for b, _m in bufs], (vbuf.cpu().numpy() if vbuf is not None else None)


@pytest.mark.parametrize("name", ["u16,u8", "i32,f32", "i64,i64,i32", "u128,u128,f32"])
def test_sort_columns(rs, torch, ctx, name):
    names = COLUMN_SETS[name]
    m = len(names)
    rng = np.random.default_rng(13)
    for n in (2, 513, 20011):
        for form, pattern in ((0, "alt"), (1, "asc"), (0, "desc")):
            desc = directions(pattern, m)
            cols = make_columns(names, n, form, seed=n + form)
            for values in (rng.integers(-2 ** 15, 2 ** 15, size=(n, 3), dtype=np.int16),  # 6 bytes: no typed width
                           rng.integers(-2 ** 31, 2 ** 31, size=(n, 10), dtype=np.int32),  # 40 bytes
                           None):
                vb = 0 if values is None else values.dtype.itemsize * values.shape[1]
                wcols, wvals, _perm = columns_reference(cols, specs_of(names), desc, values, vb)
                gcols, gvals = run_sort_columns(rs, torch, ctx, names, cols, desc, values, (name, n))
                for j in range(m):
                    assert same(gcols[j], with_guards(wcols[j]), ("column", j, name, n, pattern, form, vb))
                if vb:
                    assert same(gvals, with_guards(wvals), ("values", name, n, pattern, form, vb))
                rounds, es = INFO[name]
                assert ctx.get_info(rs.INFO_LAST_LEX) == rounds | es << 8


@pytest.mark.parametrize("tname", ["f32", "i64", "u128"])
def test_sort_columns_of_one_column_is_sort_pairs(rs, torch, ctx, tname):
    n = 20011
    rng = np.random.default_rng(17)
    cols = make_columns([tname], n, 0, seed=3)
    values = rng.integers(-2 ** 62, 2 ** 62, size=(n, 1), dtype=np.int64)
    kb, kind = specs_of([tname])[0]
    for desc in (False, True):
        gcols, gvals = run_sort_columns(rs, torch, ctx, [tname], cols, [desc], values, ("one column", tname))
        kbuf, kmid = guarded(torch, cols[0])
        vbuf, vmid = guarded(torch, values)
        t = column_tensor(torch, kmid, tname)
        t, kk = t if isinstance(t, tuple) else (t, None)
        rs.radix_sort_pairs(t, vmid.view(torch.int64), descending=desc, ctx=ctx, key_kind=kk)
        ctx.check()
        assert same(gcols[0], kbuf.cpu().numpy(), ("keys", tname, desc))
        assert same(gvals, vbuf.cpu().numpy(), ("values", tname, desc))
        wk, wv, _p = pairs_reference(cols[0], values.view(np.uint8), kb, kind, 8, desc)
        assert same(gcols[0], with_guards(wk), ("keys against the reference", tname, desc))
        assert same(gvals, with_guards(wv), ("values against the reference", tname, desc))


def test_no_rows_and_one_row_write_nothing(rs, torch, ctx):
    names = COLUMN_SETS["i64,i64,i32"]
    st = torch.cuda.current_stream().cuda_stream
    for n in (0, 1):
        cols = make_columns(names, n, 1, seed=4)
        values = np.full((n, 3), 0x1234, dtype=np.int16)
        gcols, gvals = run_sort_columns(rs, torch, ctx, names, cols, [True, False, True], values, "n <= 1")
        for j in range(3):
            assert same(gcols[j], with_guards(cols[j]), ("column", j, n))
        assert same(gvals, with_guards(values), ("values", n))
        # the C call itself (radix_sort_columns returns before it for n <= 1)
        bufs = [guarded(torch, c) for c in cols]
        vbuf, _vmid = guarded(torch, values)
        spec = [(b.data_ptr() + 64, kb, kind, d) for (b, _m), (kb, kind), d in zip(bufs, specs_of(names), [True, False, True])]
        ctx.sort_columns_device(spec, vbuf.data_ptr() + 64, 6, n, st)
        ibuf, _imid = guarded(torch, np.full(n * 8, 0xA5, dtype=np.uint8))
        ctx.lexsort_device(spec, ibuf.data_ptr() + 64, n, 8, st)
        ctx.check()
        for j in range(3):
            assert same(bufs[j][0].cpu().numpy(), with_guards(cols[j]), ("column through the C call", j, n))
        assert same(vbuf.cpu().numpy(), with_guards(values), ("values through the C call", n))
        assert same(ibuf.cpu().numpy(), with_guards(np.zeros(n, dtype="<i8")), ("index through the C call", n))


def test_refusals_with_a_context(rs, torch, ctx):
    """What the C calls refuse once they have a context: nothing is enqueued, the message names the reason."""
    t = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.full((64,), -1, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L = rs._lib.load()
    col = (rs._lib.KeyColumn * 17)(*[rs._lib.KeyColumn(t.data_ptr(), 4, 1, 0, 0) for _ in range(17)])
    h = ctx._h
    assert L.rsx_lexsort_device(h, col, 0, out.data_ptr(), 64, 8, st) == rs._lib.ERR_ARG
    assert L.rsx_lexsort_device(h, col, 17, out.data_ptr(), 64, 8, st) == rs._lib.ERR_ARG
    assert L.rsx_lexsort_device(h, None, 1, out.data_ptr(), 64, 8, st) == rs._lib.ERR_ARG
    assert L.rsx_lexsort_device(h, col, 2, out.data_ptr(), 64, 2, st) == rs._lib.ERR_ARG
    assert L.rsx_lexsort_device(h, col, 2, out.data_ptr(), 2 ** 32, 8, st) == rs._lib.ERR_UNSUPPORTED
    assert L.rsx_sort_columns_device(h, col, 2, None, 0, 2 ** 32, st) == rs._lib.ERR_UNSUPPORTED
    assert L.rsx_sort_columns_device(h, col, 2, None, 4, 64, st) == rs._lib.ERR_ARG
    assert L.rsx_sort_columns_device(h, col, 2, out.data_ptr(), 32769, 64, st) == rs._lib.ERR_ARG
    assert L.rsx_ctx_reserve_lex(h, 64, col, 2, 32769) == rs._lib.ERR_ARG
    bad = (rs._lib.KeyColumn * 2)(rs._lib.KeyColumn(t.data_ptr(), 4, 1, 0, 0), rs._lib.KeyColumn(t.data_ptr(), 4, 1, 0, 5))
    assert L.rsx_lexsort_device(h, bad, 2, out.data_ptr(), 64, 8, st) == rs._lib.ERR_ARG  # reserved
    bad[1] = rs._lib.KeyColumn(t.data_ptr(), 3, 0, 0, 0)
    assert L.rsx_lexsort_device(h, bad, 2, out.data_ptr(), 64, 8, st) == rs._lib.ERR_UNSUPPORTED
    bad[1] = rs._lib.KeyColumn(t.data_ptr(), 2, 2, 0, 0)
    assert L.rsx_lexsort_device(h, bad, 2, out.data_ptr(), 64, 8, st) == rs._lib.ERR_UNSUPPORTED
    bad[1] = rs._lib.KeyColumn(None, 4, 0, 0, 0)
    assert L.rsx_lexsort_device(h, bad, 2, out.data_ptr(), 64, 8, st) == rs._lib.ERR_ARG
    bad[1] = rs._lib.KeyColumn(t.data_ptr() + 2, 4, 0, 0, 0)
    assert L.rsx_lexsort_device(h, bad, 2, out.data_ptr(), 64, 8, st) == rs._lib.ERR_ARG
    ctx.check()
    assert bool((out == -1).all()) and bool((t == 0).all())
    ctx.reserve_lex(4096, [(0, 8, 1, False), (0, 8, 1, True), (0, 4, 1, False)], 40)
