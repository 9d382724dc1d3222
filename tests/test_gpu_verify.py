"""GPU: rsx_verify_device -- the only judge of every test too large for the CPU oracle -- against the numpy restatement
of its three words (util.verify_reference: descents, multiset checksum, stability violations).  All three words must
be equal, for every layout, on sorted and unsorted input, at the sizes where the kernel's grid-stride loop and its
workgroups end, and with single defects planted in otherwise sorted arrays.  Exact: integers compared with ==."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

U, S, F = util.UNSIGNED, util.SIGNED, util.FLOAT
LAYOUTS = [(t, util.TYPES[t]) for t in util.TYPES] + [("any%d-%d-%d" % L[:3], L) for L in util.ANY_LAYOUTS]
IDS = [x[0] for x in LAYOUTS]
GUARD = 64


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
    c = rs.Context(torch.cuda.current_device())
    yield c
    c.close()


@pytest.fixture(scope="module")
def stride(rs, ctx):
    """Threads of the verifier's largest grid: blocks are capped at 16 per CU, 256 threads each."""
    return 16 * ctx.get_info(rs._lib.INFO_NUM_CU) * 256


def _input(name, lay, n, dist, seed):
    return util.make_input(name, n, dist, seed) if name in util.TYPES else util.make_input_layout(lay, n, dist, seed)


def _words(torch, ctx, rs, x, n, lay):
    """The three words of rsx_verify_device for the n elements at tensor x, as python ints (unsigned)."""
    out = torch.full((3,), -1, dtype=torch.int64, device="cuda")  # stale contents must not matter
    ctx.verify_device(x.data_ptr() if n else 0, n, rs.RadixDigits(*lay), out.data_ptr())
    ctx.check()
    return tuple(int(v) for v in out.cpu().numpy().astype(np.uint64))


def _device_words(torch, ctx, rs, raw, lay, offset=0):
    """raw copied into device memory at byte `offset` of a buffer of its own, guard bytes behind it."""
    buf = torch.full((offset + raw.size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[offset:offset + raw.size] = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
    return _words(torch, ctx, rs, buf[offset:], raw.size // lay[0], lay)


def _check(torch, ctx, rs, orc, raw, lay, what, offset=0):
    want = util.verify_reference(raw, lay, orc)
    got = _device_words(torch, ctx, rs, raw, lay, offset)
    assert got == want, (what, "device", got, "reference", want)
    return want


@pytest.mark.parametrize("name,lay", LAYOUTS, ids=IDS)
def test_every_layout_unsorted_and_sorted(rs, torch, ctx, orc, name, lay):
    """Every util.TYPES entry and the any-layouts, on unsorted input and on its sorted form, at offset 0 and at an odd
    offset (three elements in for layouts with sort kernels of their own, three bytes in for the others)."""
    es = lay[0]
    odd = 3 if name not in util.TYPES else 3 * es
    n = 16385
    for i, dist in enumerate(("uniform", "two", "zipf", "reversed")):
        raw = _input(name, lay, n, dist, seed=200 + i)  # f32 / f64 uniform: NaNs, infinities, +-0, denormals included
        srt = orc.sort_parallel(raw, orc.Layout(*lay), 4)
        for offset in (0, odd):
            w = _check(torch, ctx, rs, orc, raw, lay, (name, dist, offset, "unsorted"), offset)
            s = _check(torch, ctx, rs, orc, srt, lay, (name, dist, offset, "sorted"), offset)
            assert s[0] == 0 and s[1] == w[1], (name, dist)
            if dist == "uniform":
                assert w[0] > n // 4


@pytest.mark.parametrize("name,lay", LAYOUTS, ids=IDS)
def test_small_sizes(rs, torch, ctx, orc, name, lay):
    for n in (0, 1, 2, 255, 256, 257, 16385):
        for dist in ("uniform", "reversed"):
            _check(torch, ctx, rs, orc, _input(name, lay, n, dist, seed=300 + n), lay, (name, n, dist))


def test_elements_of_32768_bytes(rs, torch, ctx, orc):
    """RSX_MAX_ELEM_BYTES: 600 elements of 32768 random bytes (the checksum chain runs over every one of them), the key in
    the first 8 and the index behind it, unsorted and sorted, at offset 0 and three bytes in."""
    lay = (32768, 0, 8, U)
    n = 600
    rng = np.random.default_rng(32768)
    raw = rng.integers(0, 256, size=(n, 32768), dtype=np.uint8)
    raw[:, 0:8] = util._key_ints("step16", n, 8, rng)
    raw[:, 8:16] = np.arange(n, dtype="<u8").view(np.uint8).reshape(n, 8)
    raw = raw.reshape(-1)
    srt = orc.sort_parallel(raw, orc.Layout(*lay), 4)
    w = _check(torch, ctx, rs, orc, raw, lay, "32768 unsorted")
    s = _check(torch, ctx, rs, orc, srt, lay, "32768 sorted", offset=3)
    assert w[0] > n // 4 and s[0] == 0 and s[2] == 0 and s[1] == w[1]
    bad = srt.copy()
    bad[-1] ^= 0x80  # the last byte of the last element: only that element's hash moves
    moved = (s[1] - util.element_hash_int(srt[-32768:]) + util.element_hash_int(bad[-32768:])) & ((1 << 64) - 1)
    assert moved != s[1] and _device_words(torch, ctx, rs, bad, lay) == (0, moved, 0)


@pytest.mark.parametrize("name", ["u32", "f64", "(u64,u64)", "(u128,u128)", "any7-1-6"])
def test_sizes_above_the_grid_cap(rs, torch, ctx, orc, stride, name):
    """More elements than the largest grid has threads: the grid-stride loop takes a second and a third turn; one
    size a multiple of 256, one not."""
    lay = dict(LAYOUTS)[name]
    for n, dist in ((2 * stride + 512, "uniform"), (2 * stride + 512 + 77, "two")):
        raw = _input(name, lay, n, dist, seed=400)
        _check(torch, ctx, rs, orc, raw, lay, (name, n, dist, "unsorted"))
        _check(torch, ctx, rs, orc, orc.sort_parallel(raw, orc.Layout(*lay), 8), lay, (name, n, dist, "sorted"))


def _swap(a, i, j):
    a[[i, j]] = a[[j, i]]


def test_single_descents_at_the_edges(rs, torch, ctx, orc, stride):
    """ONE descent planted in a sorted array of distinct keys: first pair, last pair, across a workgroup edge, across
    the first and the second end of the grid's stride.  Every one must be counted, once."""
    name, lay = "(u64,u64)", util.TYPES["(u64,u64)"]
    n = 2 * stride + 1000
    srt = orc.sort_parallel(util.make_input(name, n, "uniform", seed=11), orc.Layout(*lay), 8).reshape(n, 16)
    clean = _check(torch, ctx, rs, orc, srt.reshape(-1), lay, "clean")
    assert clean[0] == 0 and clean[2] == 0
    for i in (0, n - 2, 255, stride - 1, 2 * stride - 1, n // 2):
        bad = srt.copy()
        _swap(bad, i, i + 1)
        want = _check(torch, ctx, rs, orc, bad.reshape(-1), lay, ("descent at", i))
        assert want == (1, clean[1], 0), (i, want)  # (the reference agrees that this is one descent and nothing else)


def test_last_pair_at_every_residue(rs, torch, ctx, orc):
    """The pair (n-2, n-1) for sizes around a workgroup: the last pair of the array is never dropped."""
    name, lay = "u32", util.TYPES["u32"]
    for n in (2, 3, 64, 65, 256, 257, 258, 511, 512, 513):
        srt = orc.sort_parallel(util.make_input(name, n, "uniform", seed=n), orc.Layout(*lay), 1).reshape(n, 4)
        _swap(srt, n - 2, n - 1)
        want = _check(torch, ctx, rs, orc, srt.reshape(-1), lay, ("last pair", n))
        assert want[0] == 1


def test_equal_neighbours_swapped_is_instability_only(rs, torch, ctx, orc, stride):
    for name in ("(u32,u32)", "(u64,u64)", "(pay64+f64)", "(u128,u128)", "(u8,[u8;7])"):
        lay = util.TYPES[name]
        es, ko, kb, _ = lay
        n = stride + 300
        srt = orc.sort_parallel(util.make_input(name, n, "two", seed=12), orc.Layout(*lay), 8).reshape(n, es)
        clean = _check(torch, ctx, rs, orc, srt.reshape(-1), lay, (name, "clean"))
        assert clean[0] == 0 and clean[2] == 0
        key = srt[:, ko:ko + kb]
        same = np.flatnonzero((key[:-1] == key[1:]).all(axis=1))
        for i in (int(same[0]), int(same[same >= stride - 1][0]), int(same[-1])):
            bad = srt.copy()
            _swap(bad, i, i + 1)
            want = _check(torch, ctx, rs, orc, bad.reshape(-1), lay, (name, "equal keys swapped at", i))
            assert want == (0, clean[1], 1), (name, i, want)


def test_lost_and_duplicated_element_moves_the_checksum_only(rs, torch, ctx, orc):
    for name, lay in LAYOUTS:
        es = lay[0]
        n = 5000
        srt = orc.sort_parallel(_input(name, lay, n, "uniform", seed=13), orc.Layout(*lay), 2).reshape(n, es)
        clean = util.verify_reference(srt.reshape(-1), lay, orc)
        i = 2500
        if (srt[i] == srt[i + 1]).all():
            continue  # (one-byte elements: the neighbour is the same element)
        bad = srt.copy()
        bad[i] = bad[i + 1]  # element i lost, element i + 1 twice: still in order
        want = _check(torch, ctx, rs, orc, bad.reshape(-1), lay, (name, "duplicate"))
        assert want[0] == 0 and want[1] != clean[1], (name, want, clean)
        if clean[2] == 0:  # (one-byte payloads wrap at this n and count as violations before and after)
            assert want[2] == 0, (name, want)


@pytest.mark.parametrize("name", ["(u128,u128)", "any100-36-16", "any40-0-8", "(u64,[u64;2])", "(u32,[u8;8])"])
def test_one_bit_anywhere_in_a_wide_element_moves_the_checksum(rs, torch, ctx, orc, name):
    """The checksum covers every byte of the element, the last payload byte included (which neither the order nor
    the stability word looks at)."""
    lay = dict(LAYOUTS)[name]
    es, ko, kb, _ = lay
    n = 3001
    srt = orc.sort_parallel(_input(name, lay, n, "uniform", seed=14), orc.Layout(*lay), 2).reshape(n, es)
    clean = _check(torch, ctx, rs, orc, srt.reshape(-1), lay, (name, "clean"))
    pay = [b for b in range(es) if not ko <= b < ko + kb]
    seen = {clean[1]}
    for byte in sorted({pay[0], pay[7], pay[8] if len(pay) > 8 else pay[-1], pay[-1], es - 1}):
        for bit in (0, 7):
            bad = srt.copy()
            bad[n - 1 if byte == es - 1 else n // 2, byte] ^= 1 << bit
            want = _check(torch, ctx, rs, orc, bad.reshape(-1), lay, (name, "bit", byte, bit))
            assert want[0] == 0 and want[1] not in seen, (name, byte, bit, want)
            seen.add(want[1])
            if pay.index(byte) >= 8:
                assert want[2] == 0  # beyond the eight payload bytes that the stability word reads


@pytest.mark.parametrize("name", ["u128", "i128", "(u128,u128)", "any100-36-16"])
def test_high_half_of_a_16_byte_key_orders(rs, torch, ctx, orc, name):
    """Keys whose low halves ascend and whose high halves are equal; one bit set in byte 15 of one key: a descent
    that only the high 64 bits show.  And keys that differ in the high half only."""
    lay = dict(LAYOUTS)[name]
    es, ko, kb, _ = lay
    n = 4000
    srt = _input(name, lay, n, "sorted", seed=0).reshape(n, es)  # key = index: high half zero
    clean = _check(torch, ctx, rs, orc, srt.reshape(-1), lay, (name, "clean"))
    assert clean[0] == 0
    for i, byte, bit in ((n // 2, 15, 0), (255, 15, 6), (0, 8, 0), (n - 2, 12, 3)):
        bad = srt.copy()
        bad[i, ko + byte] ^= 1 << bit
        want = _check(torch, ctx, rs, orc, bad.reshape(-1), lay, (name, "high-half bit", i, byte, bit))
        assert want[0] == 1, (name, i, want)
    hi_only = srt.copy()
    hi_only[:, ko + 8:ko + 16] = hi_only[:, ko:ko + 8][::-1]  # high halves descend, low halves ascend
    hi_only[:, ko + 15] = 0
    want = _check(torch, ctx, rs, orc, hi_only.reshape(-1), lay, (name, "high halves descend"))
    assert want[0] == n - 1


def _elems(lay, keys, payload0=0):
    """Elements of layout `lay` from raw key bit patterns (python ints), payload = position."""
    es, ko, kb, _ = lay
    raw = np.zeros((len(keys), es), dtype=np.uint8)
    for i, k in enumerate(keys):
        raw[i, ko:ko + kb] = np.frombuffer((k & ((1 << (8 * kb)) - 1)).to_bytes(kb, "little"), dtype=np.uint8)
        pay = [b for b in range(es) if not ko <= b < ko + kb]
        if pay:
            raw[i, pay[0]] = payload0 + i
    return raw.reshape(-1)


def test_float_zeros_and_specials(rs, torch, ctx, orc):
    """total_cmp order: -0.0 sorts below +0.0, -NaN below -inf, +inf below +NaN."""
    for name, kb in (("f32", 4), ("f64", 8), ("(f32,u32)", 4), ("(pay64+f64)", 8)):
        lay = util.TYPES[name]
        top = 1 << (8 * kb - 1)
        inf = (0xFF << 23) if kb == 4 else (0x7FF << 52)
        nan = inf | 1
        for keys, descents in (((top, 0), 0), ((0, top), 1), ((top | nan, top | inf), 0), ((top | inf, top | nan), 1),
                               ((inf, nan), 0), ((nan, inf), 1), ((top | 1, 1), 0), ((1, top | 1), 1),
                               ((top | nan, top | inf, top | 1, top, 0, 1, inf, nan), 0)):
            want = _check(torch, ctx, rs, orc, _elems(lay, keys), lay, (name, [hex(k) for k in keys]))
            assert want[0] == descents, (name, keys, want)


def test_signed_pairs_across_zero(rs, torch, ctx, orc):
    for name, lay in [(t, util.TYPES[t]) for t in ("i8", "i16", "i32", "i64", "i128", "isize", "(i16,u16)")] + \
                     [("any7-1-6", (7, 1, 6, S))]:
        kb = lay[2]
        lowest = 1 << (8 * kb - 1)
        for keys, descents in (((-1, 0), 0), ((0, -1), 1), ((lowest, -1, 0, 1, lowest - 1), 0), ((lowest - 1, lowest), 1),
                               ((-2, -1), 0), ((-1, -2), 1)):
            want = _check(torch, ctx, rs, orc, _elems(lay, keys), lay, (name, keys))
            assert want[0] == descents, (name, keys, want)


def test_d_out_is_overwritten_not_accumulated(rs, torch, ctx, orc):
    name, lay = "(u32,u32)", util.TYPES["(u32,u32)"]
    d = rs.RadixDigits(*lay)
    n = 70001
    raw = util.make_input(name, n, "reversed", seed=1)
    raw.reshape(n, 8)[:, 4:] = raw.reshape(n, 8)[::-1, 4:]  # payloads descend too
    want = util.verify_reference(raw, lay, orc)
    x = torch.from_numpy(raw).cuda()
    out = torch.zeros(3, dtype=torch.int64, device="cuda")
    for _ in range(2):  # the second call on the same words gives the same words
        ctx.verify_device(x.data_ptr(), n, d, out.data_ptr())
        assert tuple(int(v) for v in out.cpu().numpy().astype(np.uint64)) == want
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctx.verify_device(x.data_ptr(), n, d, out.data_ptr(), side.cuda_stream)
    side.synchronize()
    assert tuple(int(v) for v in out.cpu().numpy().astype(np.uint64)) == want
    # n == 0 with a null data pointer: three zero words, whatever d_out held
    ctx.verify_device(0, 0, d, out.data_ptr())
    assert out.cpu().tolist() == [0, 0, 0]
    with pytest.raises(rs.RsxError):
        ctx.verify_device(x.data_ptr(), n, d, 0)
    with pytest.raises(rs.RsxError):
        ctx.verify_device(0, n, d, out.data_ptr())


def _sum_hash(counts):
    """sum of count * hash(element) mod 2^64 for {element bytes: count}."""
    return sum(c * util.element_hash_int(e) for e, c in counts.items()) & ((1 << 64) - 1)


def test_more_than_2pow32_bytes(rs, torch, ctx, orc):
    """(u8,[u8;7]), 2^29 + 1001 elements (byte offsets beyond 2^32), all equal (GEN_CONSTANT, zero payload), then
    defects in the last 16 elements.  Expected words by arithmetic: n x hash(fill) adjusted for the planted tail."""
    name, lay = "(u8,[u8;7])", util.TYPES["(u8,[u8;7])"]
    d = rs.RadixDigits(*lay)
    n = (1 << 29) + 1001
    x = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    ctx.generate_device(x.data_ptr(), n, d, rs.GEN_CONSTANT | rs.GEN_PAYLOAD_ZERO, 1, 9.0)
    fill = bytes([9, 0, 0, 0, 0, 0, 0, 0])
    assert bytes(x[-8:].cpu().numpy()) == fill and bytes(x[:8].cpu().numpy()) == fill
    assert _words(torch, ctx, rs, x, n, lay) == (0, _sum_hash({fill: n}), 0)
    tail = np.frombuffer(fill * 16, dtype=np.uint8).reshape(16, 8).copy()
    tail[3, 0] = 200          # a descent behind it
    tail[7, 1:] = 5           # equal keys, payload 0x05050505050505 then 0: one stability violation
    tail[14, 7] = 1           # the top payload byte counts: a violation at (14, 15)
    tail[15, 0] = 9
    x[-16 * 8:] = torch.from_numpy(tail.reshape(-1)).cuda()
    head = np.frombuffer(fill, dtype=np.uint8)  # element n - 17, joined to the tail for the pair (n-17, n-16)
    t = util.verify_reference(np.concatenate([head, tail.reshape(-1)]), lay, orc)
    want = (t[0], (_sum_hash({fill: n - 17}) + t[1]) & ((1 << 64) - 1), t[2])
    assert t[0] == 1 and t[2] == 2
    assert _words(torch, ctx, rs, x, n, lay) == want
    del x
    torch.cuda.empty_cache()


def test_more_than_2pow32_elements(rs, torch, ctx, orc):
    """u8, 2^32 + 1000 elements, key = index mod 256 (GEN_SORTED): a descent after every 256 elements, counted beyond
    2^32; the checksum from the count of every byte value; then defects in the last elements."""
    lay = util.TYPES["u8"]
    d = rs.RadixDigits(*lay)
    n = (1 << 32) + 1000
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.generate_device(x.data_ptr(), n, d, rs.GEN_SORTED, 1)
    assert x[-3:].cpu().tolist() == [(n - 3) & 255, (n - 2) & 255, (n - 1) & 255] and x[:2].cpu().tolist() == [0, 1]

    def closed_form(m):  # elements 0 .. m-1 of the fill
        counts = {bytes([v]): m // 256 + (1 if v < m % 256 else 0) for v in range(256)}
        return (m - 1) // 256, _sum_hash(counts), 0  # pairs (i, i+1) with i % 256 == 255 and i + 1 < m

    assert _words(torch, ctx, rs, x, n, lay) == closed_form(n)
    tail = np.array([(n - 16 + i) & 255 for i in range(16)], dtype=np.uint8)
    tail[15] = 0              # descent at the very last pair
    tail[5] = 255             # and one inside
    x[-16:] = torch.from_numpy(tail).cuda()
    head = np.array([(n - 17) & 255], dtype=np.uint8)
    t = util.verify_reference(np.concatenate([head, tail]), lay, orc)
    c = closed_form(n - 17)   # (n - 17) % 256 != 0: no descent of the fill between elements n-18 and n-17
    assert (n - 18) % 256 != 255 and t[0] == 2
    assert _words(torch, ctx, rs, x, n, lay) == (c[0] + t[0], (c[1] + t[1]) & ((1 << 64) - 1), 0)
    del x
    torch.cuda.empty_cache()
