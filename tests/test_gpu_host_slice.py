"""GPU: rsx_sort_host, the `&mut [T]` drop-in, past one staging chunk.

The copies of rsx_sort_host are a hand-written pipeline (host_pipeline and par_memcpy in radix_sort_amd/csrc/rsx.hip):
pieces of one chunk go over a ring of four pinned buffers, one event per slot guards its reuse, a threaded memcpy splits
a piece of 4 MiB and more at 4096-byte steps, and the drain of the copy back runs four pieces behind its DMA.  At the
shipped chunk of 32 MiB all of that starts at 128 MiB, so RSX_OPT_HOST_CHUNK shortens the pieces and the tests below
reach every branch with arrays of a few KB: one chunk, the ring exactly full, the first reuse of a slot, the second lap
full, its reuse, a short last piece, elements that straddle two pieces.

Every result is compared whole, byte for byte, with a CPU reference (the oracle for the layouts, numpy's stable sorts
where they are cheap).  Every host array lies inside a larger uint8 allocation of the test's own filled with 0xA5, at
least 4096 bytes of it in front and behind, and the whole allocation outside the array is checked after every sort: the
pipeline writes host memory with plain memcpy, so an overrun is silent otherwise.

What these tests do NOT prove: that the per-slot event waits are there.  A missing wait (or a slot reused one piece
early) is a race between a memcpy and a DMA; small pieces make it likely to show, not certain.  Wrong offsets, lengths
and slots in the copy back, and overruns, are caught deterministically."""
import threading
import time

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

U = util.UNSIGNED
MIB = 1 << 20
DEFAULT_CHUNK = 32 * MIB
GUARD = 4096
# the layouts without kernels of their own, as test_gpu_any_layout.py builds them: route 1 (packed re-layout) and
# route 2 (key-index proxy, whose gather reads the second staging array)
ANY = {"any6/2": (6, 0, 2, U), "any40/8": (40, 0, 8, U)}
EDGE_TYPES = ["u8", "u32", "u64", "f64", "(u32,u32)", "(u64,u64)", "(u32,[u8;8])", "u128", "(u128,u128)"] + list(ANY)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def rs():
    import radix_sort_amd as rs
    return rs


@pytest.fixture()
def ctx(rs, torch):
    c = rs.Context(torch.cuda.current_device())
    yield c
    c.close()


def layout_of(t):
    return ANY[t] if t in ANY else util.TYPES[t]


def make(t, n, dist, seed):
    """Raw bytes of n elements: the key drawn by util, every other byte the element's index (instability shows)."""
    return util.make_input_layout(ANY[t], n, dist, seed) if t in ANY else util.make_input(t, n, dist, seed)


class Guarded:
    """A copy of `raw` inside a larger uint8 allocation of 0xA5: at least `guard` bytes in front of and behind it, the
    array itself `shift` bytes past a 4096-byte boundary."""

    def __init__(self, raw, guard=GUARD, shift=0):
        raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        self.buf = np.full(guard + 4096 + raw.size + guard, 0xA5, dtype=np.uint8)
        self.start = guard + (shift - (self.buf.ctypes.data + guard)) % 4096
        self.size = raw.size
        self.a = self.buf[self.start:self.start + self.size]
        self.a[:] = raw
        assert self.a.ctypes.data % 4096 == shift and self.start >= guard and self.buf.size - self.start - self.size >= guard

    def check(self, what=""):
        front, back = self.buf[:self.start], self.buf[self.start + self.size:]
        assert (front == 0xA5).all(), f"bytes in front of the slice were written {what}"
        assert (back == 0xA5).all(), f"bytes behind the slice were written {what}"


def host_sort(rs, c, raw, lay, guard=GUARD, shift=0):
    """radix_sort of a guarded copy of raw on context c; returns the sorted bytes after the guards were checked."""
    g = Guarded(raw, guard, shift)
    es = lay[0]
    rs.radix_sort(g.a.reshape(-1, es), digits=rs.RadixDigits(*lay), ctx=c)  # (n, elem_bytes): the array states its element
    g.check((lay, raw.size // es))
    return g.a


def edge_sizes(chunk, es):
    """n = floor(k C / es) + d: one chunk, the ring exactly full, the first slot reuse, the second lap full, its reuse,
    each one element short, exact and one element over.  Largest first: the context's staging arrays then exceed every
    later array, so a copy back that takes a whole chunk for the short last piece has bytes to take."""
    return [(k, d, k * chunk // es + d) for k in (9, 8, 5, 4, 1) for d in (1, 0, -1)]


# ---- a. chunk edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [4096, 65536])
@pytest.mark.parametrize("t", EDGE_TYPES)
def test_chunk_edges(rs, ctx, orc, t, chunk):
    lay = layout_of(t)
    es = lay[0]
    ctx.set_option(rs.OPT_HOST_CHUNK, chunk)
    # a wrong chunk index in the copy back lands up to four chunks behind the slice: guards that hold it
    guard = max(GUARD, 5 * chunk)
    for dist in ("uniform", "step16"):
        for k, d, n in edge_sizes(chunk, es):
            raw = make(t, n, dist, seed=100 * k + d + 7)
            want = orc.sort_parallel(raw, orc.Layout(*lay), 4)
            got = host_sort(rs, ctx, raw, lay, guard)
            assert np.array_equal(got, want), (t, chunk, dist, k, d, n)
            if t in ("u32", "u64"):  # a second, independent reference where it is cheap
                dt = "<u4" if t == "u32" else "<u8"
                assert np.array_equal(got.view(dt), np.sort(raw.view(dt), kind="stable"))
            elif t in ("(u32,u32)", "(u64,u64)"):
                dt = "<u4" if t == "(u32,u32)" else "<u8"
                e = raw.view(dt).reshape(n, 2)
                assert np.array_equal(got.view(dt).reshape(n, 2), e[np.argsort(e[:, 0], kind="stable")])


def test_elements_straddle_the_chunks():
    """What the 12-, 6- and 40-byte cases above are for: their elements do not divide a chunk."""
    for chunk in (4096, 65536):
        for es in (6, 12, 40):
            assert chunk % es != 0
    assert DEFAULT_CHUNK % 12 != 0 and DEFAULT_CHUNK % 16 == 0


# ---- b. the threaded copy ----------------------------------------------------------------------------------------
def _numpy_case(t, n, seed):
    """(raw bytes, expected bytes) by numpy: u32 keys from 2^20 values, (u64, u64) with 50 keys and the index behind."""
    rng = np.random.default_rng(seed)
    if t == "u32":
        a = rng.integers(0, 1 << 20, size=n, dtype=np.uint32)
        return a.view(np.uint8), np.sort(a, kind="stable").view(np.uint8)
    e = np.empty((n, 2), dtype=np.uint64)
    e[:, 0] = rng.integers(0, 50, size=n, dtype=np.uint64)
    e[:, 1] = np.arange(n, dtype=np.uint64)
    return e.reshape(-1).view(np.uint8), e[np.argsort(e[:, 0], kind="stable")].reshape(-1).view(np.uint8)


THREADED_CHUNKS = [4 * MIB, 8 * MIB - 4096]


def _threaded_sizes(chunk, es):
    """bytes of the arrays of test_threaded_copy for one chunk size."""
    out = {"k5+1": (5 * chunk // es + 1) * es,  # five whole chunks through par_memcpy's split, one element behind
           "tail C/2+es": 4 * chunk + chunk // 2 + es}  # slot 0 reused by a tail of half a chunk and one element
    if chunk > 4 * MIB + 4096 + es:
        # C/2 + es stays under par_memcpy's 4 MiB threshold for every chunk up to 8 MiB, so that tail is one memcpy: a tail
        # that is itself split, with a remainder for the last thread, is 4 MiB + 4096 + es
        out["tail 4MiB+4096+es"] = 4 * chunk + 4 * MIB + 4096 + es
        # ... and 4 MiB + es: for 4-byte elements bytes / 8 threads is a multiple of 4096 with 4 bytes left over, which
        # par_memcpy once dropped (it rounded the quotient down before rounding it to 4096)
        out["tail 4MiB+es"] = 4 * chunk + 4 * MIB + es
    return out


@pytest.mark.parametrize("chunk", THREADED_CHUNKS)
@pytest.mark.parametrize("t", ["u32", "(u64,u64)"])
def test_threaded_copy(rs, ctx, t, chunk):
    """par_memcpy: a chunk of 4 MiB splits evenly over the threads; at 8 MiB - 4096, bytes / threads is no multiple of
    4096 for 2, 4 and 8 threads, so the last thread gets a remainder."""
    lay = util.TYPES[t]
    es = lay[0]
    for threads in (2, 4, 8):
        assert (4 * MIB // threads) % 4096 == 0 and ((8 * MIB - 4096) // threads) % 4096 != 0
    ctx.set_option(rs.OPT_HOST_CHUNK, chunk)
    for name, nbytes in _threaded_sizes(chunk, es).items():
        assert nbytes % es == 0 and -(-nbytes // chunk) == (6 if name == "k5+1" else 5)
        raw, want = _numpy_case(t, nbytes // es, seed=len(name))
        assert np.array_equal(host_sort(rs, ctx, raw, lay), want), (t, chunk, name)


# ---- c. the shipped configuration, once ----------------------------------------------------------------------------
MULT = 2654435761  # a prime above every n below: i -> i * MULT mod n is a permutation of 0 .. n-1


def _permutation(n):
    assert n < MULT and (n - 1) * MULT < 1 << 64
    return (np.arange(n, dtype=np.uint64) * np.uint64(MULT)) % np.uint64(n)


def test_default_chunk_u32(rs, ctx):
    """The option untouched: u32 at 5 x 32 MiB + 4 MiB + 4 bytes -- slot 0 reused by a tail that par_memcpy splits with a
    remainder.  The keys are a permutation of 0 .. n-1, so the expected result is arange(n) and no CPU sort runs.
    Measured on an MI355X machine: making the input 0.23 s, the sort (the copy into the guarded allocation and the guard
    check included) 0.03 s."""
    nbytes = 5 * DEFAULT_CHUNK + 4 * MIB + 4
    n = nbytes // 4
    t0 = time.perf_counter()
    raw = _permutation(n).astype(np.uint32)
    t1 = time.perf_counter()
    got = host_sort(rs, ctx, raw, util.TYPES["u32"])
    t2 = time.perf_counter()
    print(f"default chunk u32: n={n} input {t1 - t0:.2f} s, sort with guard check {t2 - t1:.2f} s")
    assert np.array_equal(got.view("<u4"), np.arange(n, dtype=np.uint32))


def test_default_chunk_pairs_with_ties(rs, ctx):
    """The option untouched: (u64, u64) at 5 x 32 MiB + 16 bytes -- slot 0 reused by one element.  Key: the permutation
    divided by 8 (eight-way ties); payload: the index; reference: np.argsort(kind="stable") of the keys.
    Measured on an MI355X machine: the reference 0.88 s, the sort (the copy into the guarded allocation and the guard
    check included) 0.03 s -- so the size stays at five chunks and one element."""
    nbytes = 5 * DEFAULT_CHUNK + 16
    n = nbytes // 16
    e = np.empty((n, 2), dtype=np.uint64)
    e[:, 0] = _permutation(n) // np.uint64(8)
    e[:, 1] = np.arange(n, dtype=np.uint64)
    t0 = time.perf_counter()
    want = e[np.argsort(e[:, 0], kind="stable")]
    t1 = time.perf_counter()
    got = host_sort(rs, ctx, e.reshape(-1), util.TYPES["(u64,u64)"])
    t2 = time.perf_counter()
    print(f"default chunk (u64,u64): n={n} reference {t1 - t0:.2f} s, sort with guard check {t2 - t1:.2f} s")
    assert np.array_equal(got.view("<u8").reshape(n, 2), want)


# ---- d. alignment and degenerate slices ------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ["u32", "(u8,u8)"])
def test_host_pointer_one_byte_past_a_page(rs, ctx, orc, t):
    """The C ABI takes any void *: ctx.sort_host on a view that starts 1 byte past a 4096-byte boundary."""
    lay = util.TYPES[t]
    es = lay[0]
    ctx.set_option(rs.OPT_HOST_CHUNK, 65536)
    for n in (9 * 65536 // es + 1, 4 * 65536 // es, 1001):
        raw = util.make_input(t, n, "uniform", seed=n)
        g = Guarded(raw, guard=5 * 65536, shift=1)
        assert g.a.ctypes.data % 4096 == 1
        ctx.sort_host(g.a.ctypes.data, n, rs.RadixDigits(*lay))
        g.check((t, n))
        assert np.array_equal(g.a, orc.sort_parallel(raw, orc.Layout(*lay), 4)), (t, n)


def test_empty_and_single_element_slices(rs, ctx):
    """n = 0 and n = 1, with a null pointer and with a real one: success, and nothing is written."""
    for t in ("u32", "(u64,u64)", "any40/8"):
        lay = layout_of(t)
        d = rs.RadixDigits(*lay)
        for n in (0, 1):
            ctx.sort_host(0, n, d)  # NULL
            raw = make(t, 1, "uniform", seed=3)
            g = Guarded(raw)
            before = g.buf.copy()
            ctx.sort_host(g.a.ctypes.data, n, d)
            assert np.array_equal(g.buf, before), (t, n)
    with pytest.raises(rs.RsxError) as e:  # two elements behind a null pointer are refused, not read
        ctx.sort_host(0, 2, rs.RadixDigits(*util.TYPES["u32"]))
    assert e.value.status == rs._lib.ERR_ARG


def test_read_only_and_strided_arrays_are_refused(rs, ctx):
    """radix_sort refuses a read-only or non-contiguous numpy array before any copy: the array is as it was."""
    a = np.random.default_rng(5).integers(0, 2 ** 32, size=20001, dtype=np.uint32)
    keep = a.copy()
    ro = a.view()
    ro.flags.writeable = False
    for bad in (ro, a[::2], a.reshape(3, 6667).T):
        with pytest.raises(ValueError):
            rs.radix_sort(bad, ctx=ctx)
        assert np.array_equal(a, keep)
    assert ctx.get_info(rs.INFO_LAST_PASSES) == 0  # and no sort was enqueued


# ---- e. one context, several uses ----------------------------------------------------------------------------------
def test_one_context_host_and_device_sorts_in_turn(rs, torch, orc):
    """On ONE context with 64 KiB chunks: a 9-chunk host sort, a 1-chunk one, a 9-chunk one of a wider type and more bytes
    (the staging arrays grow), a device-resident sort on a side stream with a host sort behind it and no check() between
    them (the host path must wait for the device sort on its own: they share the workspace), a device-resident sort after
    a host sort -- then the same steps in reverse order.  Every result against the oracle."""
    C = 65536
    c = rs.Context(torch.cuda.current_device())
    c.set_option(rs.OPT_HOST_CHUNK, C)
    side = torch.cuda.Stream()

    def host(t, n, dist, seed):
        lay = util.TYPES[t]
        raw = util.make_input(t, n, dist, seed=seed)
        got = host_sort(rs, c, raw, lay, guard=5 * C)
        assert np.array_equal(got, orc.sort_parallel(raw, orc.Layout(*lay), 4)), (t, n, dist)

    def device_start(t, n, seed, stream):
        raw = util.make_input(t, n, "uniform", seed=seed)
        x = torch.from_numpy(raw.copy()).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            rs.radix_sort(x, digits=rs.RadixDigits(*util.TYPES[t]), ctx=c)
        return raw, x, stream

    def device_finish(t, raw, x, stream):
        c.check(stream.cuda_stream)
        assert np.array_equal(x.cpu().numpy(), orc.sort_parallel(raw, orc.Layout(*util.TYPES[t]), 4)), t

    def device_then_host():
        pending = device_start("u32", 300001, 901, side)
        host("(u32,u32)", 9 * C // 8 - 2, "step16", 902)  # enqueued behind the device sort, no check() in between
        device_finish("u32", *pending)

    def host_then_device():
        host("u64", 5 * C // 8 + 1, "uniform", 903)
        device_finish("u32", *device_start("u32", 300001, 904, torch.cuda.current_stream()))

    assert 9 * C > (8 * C + 5 * 4)
    steps = [lambda: host("u32", 8 * C // 4 + 5, "uniform", 905),  # 9 chunks, the last one 20 bytes
             lambda: host("u32", C // 4 - 1, "step16", 906),  # 1 chunk
             lambda: host("(u128,u128)", 9 * C // 32, "step16", 907),  # 9 whole chunks: more bytes than before
             device_then_host, host_then_device]
    for step in steps + steps[::-1]:
        step()
    c.close()


# ---- f. two Python threads -------------------------------------------------------------------------------------------
def _threads_sort(rs, ctxs, raws, wants, lay, rounds=5, timeout=120.0):
    """Thread i host-sorts raws[i] `rounds` times on ctxs[i] (ctypes releases the GIL during the call)."""
    errors = []

    def work(i):
        try:
            for r in range(rounds):
                got = host_sort(rs, ctxs[i], raws[i], lay, guard=5 * 65536)
                if not np.array_equal(got, wants[i]):
                    errors.append(f"thread {i}, round {r}: result differs")
        except BaseException as e:  # noqa: BLE001 (reported by the test)
            errors.append(f"thread {i}: {e!r}")

    ths = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(len(raws))]
    for th in ths:
        th.start()
    deadline = time.monotonic() + timeout
    for th in ths:
        th.join(max(0.0, deadline - time.monotonic()))
    assert not any(th.is_alive() for th in ths), "a host sort did not return"
    assert not errors, errors


def test_two_threads_one_context_then_one_each(rs, torch, orc):
    """Two threads, each with its own 9-chunk array (64 KiB chunks), five sorts each: first on one shared context, whose
    mutex must serialise the ring, then on one context per thread."""
    C = 65536
    t = "(u32,u32)"
    lay = util.TYPES[t]
    raws = [util.make_input(t, 9 * C // 8 - 3 + 2 * i, dist, seed=950 + i) for i, dist in enumerate(("uniform", "step16"))]
    wants = [orc.sort_parallel(r, orc.Layout(*lay), 4) for r in raws]
    ctxs = [rs.Context(torch.cuda.current_device()) for _ in range(2)]
    for c in ctxs:
        c.set_option(rs.OPT_HOST_CHUNK, C)
    _threads_sort(rs, [ctxs[0], ctxs[0]], raws, wants, lay)
    _threads_sort(rs, ctxs, raws, wants, lay)
    for c in ctxs:
        c.close()


# ---- g. the option itself --------------------------------------------------------------------------------------------
def test_host_chunk_option_values(rs, ctx, orc):
    """Multiples of 4096 in [4096, 32 MiB] are taken; 0, 4095, 4096 + 1, 32 MiB + 4096 and 2^40 are RSX_ERR_ARG and leave
    the previous value in force: a following sort of 9 small chunks still matches."""
    lay = util.TYPES["(u32,[u8;8])"]
    raw = util.make_input("(u32,[u8;8])", 9 * 4096 // 12 + 1, "step16", seed=77)
    want = orc.sort_parallel(raw, orc.Layout(*lay), 4)
    for good in (DEFAULT_CHUNK, 8192, 32 * MIB - 4096, 4096):
        ctx.set_option(rs.OPT_HOST_CHUNK, good)
    for bad in (0, 4095, 4096 + 1, 32 * MIB + 4096, 1 << 40):
        with pytest.raises(rs.RsxError) as e:
            ctx.set_option(rs.OPT_HOST_CHUNK, bad)
        assert e.value.status == rs._lib.ERR_ARG, bad
        assert np.array_equal(host_sort(rs, ctx, raw, lay, guard=5 * 4096), want), bad
