"""The direct bucket kernel against the stable passes (RSX_OPT_BUCKET_DIRECT 1 / 0) on 2^30 u64 keys whose 16384-key
buckets consist of sub-buckets of exactly PER distinct keys each (the 12 bits below the window take 16384 / PER values):
python tools/direct_probe.py [PER ...]   -- default: 4, 16, DIRECT_LIMIT (every sub-bucket AT the limit) and DIRECT_LIMIT + 1
(every bucket handed over: the cost of the hand-over).  PER = 0: uniform keys, SEEDS sorts: what is handed over (nothing)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, radix_sort_amd as rs
import bench

LIMIT = 24  # DIRECT_LIMIT (rsx_small_kernel.hpp)
LG = int(os.environ.get("LG", "30"))
n = 1 << LG
d = bench.digits_for(rs, "u64")
for per in [int(v) for v in sys.argv[1:]] or [4, 16, LIMIT, LIMIT + 1]:
    if per == 0:  # uniform keys (the headline's generator): what does the direct kernel hand over?
        x = torch.empty(n, dtype=torch.int64, device="cuda"); tmp = torch.empty_like(x)
        ctx = rs.Context(0)
        worst = 0
        for seed in range(int(os.environ.get("SEEDS", "8"))):
            ctx.generate_device(x.data_ptr(), n, d, rs.GEN_UNIFORM, seed, 1.0)
            ctx.sort_device(x.data_ptr(), tmp.data_ptr(), n, d); torch.cuda.synchronize(); ctx.check()
            worst = max(worst, ctx.get_info(rs.INFO_LAST_DIRECT))
        print(f"u64 2^{LG}, uniform, {seed + 1} seeds: most buckets handed over in one sort: {worst}", flush=True)
        ctx.close(); del x, tmp
        continue
    i = torch.arange(n, dtype=torch.int64, device="cuda")
    i.mul_(0x9E3779B1).bitwise_and_(n - 1)  # (an odd multiplier: a permutation of the indices, so the array is not presorted)
    j = i & 16383
    key = (i >> 14) << 48  # window: 2^(LG - 14) values, 16384 keys each
    key |= (torch.div(j, per, rounding_mode="floor") * max(1, per // 4)).bitwise_and_(4095) << 36
    del j
    key |= (i * 0x5851F42D4C957F2D >> 20) & ((1 << 36) - 1)  # distinct with near certainty, in no order
    del i
    x = torch.empty_like(key); tmp = torch.empty_like(key)
    out = torch.zeros(3, dtype=torch.int64, device="cuda")
    res = []
    for direct in (1, 0):
        ctx = rs.Context(0); ctx.set_option(rs.OPT_BUCKET_DIRECT, direct)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        tot = 0.0
        for it in range(6):
            x.copy_(key)
            e0.record(); ctx.sort_device(x.data_ptr(), tmp.data_ptr(), n, d); e1.record(); torch.cuda.synchronize(); ctx.check()
            if it >= 2: tot += e0.elapsed_time(e1)
        ctx.verify_device(x.data_ptr(), n, d, out.data_ptr()); torch.cuda.synchronize()
        assert out[0].item() == 0, out.tolist()
        res.append((tot / 4, ctx.get_info(rs.INFO_LAST_DIRECT)))
        ctx.close()
    print(f"u64 2^{LG}, sub-buckets of {per}: direct {res[0][0]:8.3f} ms (left {res[0][1]})   stable passes {res[1][0]:8.3f} ms", flush=True)
    del key, x, tmp
