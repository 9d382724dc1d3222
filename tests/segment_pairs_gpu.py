"""What the GPU tests of the segmented key / value calls share (test_gpu_segment_pairs.py, test_gpu_segment_pairs_matrix.py);
a helper, no tests.

Every array the library sees sits in an allocation the test owns: GUARD bytes of 0xA5, `shift` more of them, the array,
GUARD bytes; what comes back is that whole allocation, compared with segment_pairs_ref.with_guards(expected, shift)."""
import numpy as np

import util
from segment_pairs_ref import GUARD, expected_index, segments_reference, with_guards


# ---- include/rsx.h restated: where the value sits in the joined element and how large that element is ----
def voff(kb, vb):
    a = 1 if vb == 0 else 4 if vb % 4 == 0 else 2 if vb % 2 == 0 else 1
    return (kb + a - 1) // a * a


def joined_elem(kb, vb):
    need = voff(kb, vb) + vb
    return next((z for z in (1, 2, 4, 8, 12, 16, 24, 32) if z >= need and z % kb == 0), 0)


def expected_info(kb, vb):
    """RSX_INFO_LAST_PAIRS: 3 fused per segment, 4 fused on (key, position) proxies and a gather; bits 8-15 the joined size."""
    if vb in (0, 1, 2, 4, 8, 16):
        return 3 | joined_elem(kb, vb) << 8
    return 4 | joined_elem(kb, 4) << 8


def key_dtype(torch, tname):
    return {"u8": torch.uint8, "i16": torch.int16, "i32": torch.int32, "i64": torch.int64, "f32": torch.float32,
            "f64": torch.float64, "u32": torch.uint32, "u64": torch.uint64}.get(tname)


def guarded(torch, raw, shift=0):
    """(whole allocation, view of its middle) on the GPU: guards of 0xA5 around the bytes `raw`.  The middle starts
    `shift` bytes behind a 16-byte boundary: shift = 0 gives the library a 16-byte aligned array, any other shift one
    that is aligned to the largest power of two dividing shift and to nothing more."""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    buf = torch.full((GUARD + shift + raw.size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    mid = buf[GUARD + shift:GUARD + shift + raw.size]
    assert (mid.data_ptr() - shift) % 16 == 0, "the allocator no longer returns 16-byte aligned memory"
    mid.copy_(torch.from_numpy(raw))
    return buf, mid


def key_tensor(torch, mid, tname):
    if util.TYPES[tname][2] == 16:
        return mid.view(-1, 16)
    return mid.view(key_dtype(torch, tname))


def same(got, exp, what):
    if np.array_equal(got, exp):
        return True
    w = np.nonzero(got != exp)[0] if got.shape == exp.shape else np.zeros(1, dtype=np.int64)
    print(what, f": {len(w)} bytes differ, first at byte {int(w[0]) - GUARD}, last at byte {int(w[-1]) - GUARD} of the array")
    return False


def sort_pairs(rs, torch, c, tname, keys_raw, values_raw, vb, offs, desc, max_seg_len=0, check=True, shifts=(0, 0, 0)):
    """radix_sort_segments_pairs on guarded copies -> the two whole allocations as numpy bytes (values: None without)."""
    kbuf, kmid = guarded(torch, keys_raw, shifts[0])
    n = keys_raw.size // util.TYPES[tname][2]
    vbuf = vals = None
    if vb:
        vbuf, vmid = guarded(torch, values_raw, shifts[1])
        vals = vmid.view(n, vb)
    o = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
    rs.radix_sort_segments_pairs(key_tensor(torch, kmid, tname), vals, o, descending=desc, max_seg_len=max_seg_len, ctx=c)
    if check:
        c.check()
    else:
        torch.cuda.synchronize()
    return kbuf.cpu().numpy(), (vbuf.cpu().numpy() if vb else None)


def argsort(rs, torch, c, tname, keys_raw, offs, desc, idt, max_seg_len=0, check=True, shifts=(0, 0, 0)):
    """radix_argsort_segments into an index column of 0xA5 bytes -> (key allocation, index allocation) as numpy bytes."""
    kbuf, kmid = guarded(torch, keys_raw, shifts[0])
    n = keys_raw.size // util.TYPES[tname][2]
    ib = 4 if idt == torch.int32 else 8
    ibuf, imid = guarded(torch, np.full(n * ib, 0xA5, dtype=np.uint8), shifts[2])
    out = imid.view(idt)
    o = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
    got = rs.radix_argsort_segments(key_tensor(torch, kmid, tname), o, descending=desc, out=out, max_seg_len=max_seg_len, ctx=c)
    assert got is out
    if check:
        c.check()
    else:
        torch.cuda.synchronize()
    return kbuf.cpu().numpy(), ibuf.cpu().numpy()


def check_all(rs, torch, c, tname, keys_raw, values_raw, vb, offs, desc, max_seg_len=0, index_types=None, what=None,
              shifts=(0, 0, 0), reference=segments_reference):
    """Pairs (and, with index_types, argsort) of one input against the reference, whole allocations.  shifts: how far
    behind a 16-byte boundary the keys, the values and the index start (guarded)."""
    _es, _ko, kb, kind = util.TYPES[tname]
    wk, wv, local = reference(keys_raw, values_raw, kb, kind, vb, desc, offs)
    gk, gv = sort_pairs(rs, torch, c, tname, keys_raw, values_raw, vb, offs, desc, max_seg_len, shifts=shifts)
    assert same(gk, with_guards(wk, shifts[0]), ("keys", what, desc))
    if vb:
        assert same(gv, with_guards(wv, shifts[1]), ("values", what, desc))
    for idt in index_types or ():
        ib = 4 if idt == torch.int32 else 8
        gk, gi = argsort(rs, torch, c, tname, keys_raw, offs, desc, idt, max_seg_len, shifts=shifts)
        assert same(gk, with_guards(keys_raw, shifts[0]), ("argsort changed the keys", what, desc))
        assert same(gi, with_guards(expected_index(local, ib), shifts[2]), ("index", what, desc, idt))
