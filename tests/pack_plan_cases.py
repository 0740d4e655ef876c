"""Case table of the packed-weight plan (test_pack_plan_host.py and tools/gen_pack_plans.py): which layout, how many rows, which row
stride and how many bytes the library chooses for a conv weight.  Plain data and ctypes calls that launch nothing: the size queries and
rsis_conv_pack_job_fill run on the host, so all of this works without a GPU."""
import ctypes

F32, BF16, F32_WINO = 0, 1, 3                   # RSIS_DTYPE_* of include/rsis_hip.h
DTYPES = [("f32", F32), ("bf16", BF16), ("f32_wino", F32_WINO)]

# (name, Cout, Ctot, ks, stride, pad, segs, offs, lstm_hid)
CASES = [
    # the configurations of test_gpu_ops.py::test_repack_all_equals_lazy_packs
    ("repack0_3x3_two_segs", 64, 48, 3, 1, 1, [16, 32], None, 0),
    ("repack1_1x1", 256, 64, 1, 1, 0, [64], None, 0),
    ("repack2_7x7_stem", 64, 3, 7, 2, 3, [3], None, 0),
    ("repack3_3x3_s2", 40, 24, 3, 2, 1, [24], None, 0),
    ("repack4_lstm_subset", 128, 56, 3, 1, 1, [24, 8], [0, 48], 32),
    ("repack5_3x3_odd", 130, 129, 3, 1, 1, [129], None, 0),
    ("repack6_1x1_s2", 512, 256, 1, 2, 0, [256], None, 0),
    # 3x3 / stride 2 into two destinations: the data gradient is the implicit-GEMM layout inside a buffer sized for the direct one
    ("s2_two_segs", 40, 24, 3, 2, 1, [16, 8], None, 0),
    ("wino_64_64", 64, 64, 3, 1, 1, [64], None, 0),
    # a Winograd geometry over a channel subset: the forward copy is refused
    ("wino_subset", 64, 64, 3, 1, 1, [32], [32], 0),
    ("wino_dgrad_two_segs", 64, 64, 3, 1, 1, [32, 32], None, 0),
    ("lstm_hid32_ks3", 128, 48, 3, 1, 1, [16, 32], None, 32),          # accepted under bf16
    ("lstm_hid32_ks1", 128, 48, 1, 1, 0, [48], None, 32),              # refused under bf16: no fused cell epilogue for 1x1 gates
    ("cout_not_4_hid", 100, 48, 3, 1, 1, [48], None, 32),
    ("segment_past_ctot", 64, 32, 3, 1, 1, [24, 16], None, 0),
    ("nseg_0", 64, 32, 3, 1, 1, [], None, 0),
    ("nseg_4", 64, 32, 3, 1, 1, [8, 8, 8, 8], None, 0),
    ("weight_2_31_elements", 65536, 32768, 1, 1, 0, [32768], None, 0),
    ("1x1_s2", 64, 32, 1, 2, 0, [32], None, 0),
    ("7x7_s2_p3", 32, 8, 7, 2, 3, [8], None, 0),
]


def plan_id(name, dtype_name, dgrad):
    return "%s/%s/%s" % (name, dtype_name, "dgrad" if dgrad else "fwd")


def written_bytes(imode, krows, ldw):
    """bytes a pack of this plan writes: f32 rows (modes 0-4), 16-byte bf16 cells (5-6), (32 x 8)-channel blocks of 16 Winograd
    positions (7-8, where krows counts the blocks)"""
    if imode <= 4:
        return krows * ldw * 4
    if imode <= 6:
        return krows * ldw * 16
    return krows * 32 * 8 * 16 * 4


def record(L, PackJob, case, dtype, dgrad):
    """what the library answers for one case: job_fill's return value and derived fields, and both size queries"""
    _name, Cout, Ctot, ks, stride, pad, segs, offs, hid = case
    j = PackJob()
    j.W, j.out = 64, 128                          # dummy non-null addresses: nothing is launched
    j.dgrad, j.dtype, j.Cout, j.Ctot, j.ks, j.stride, j.pad, j.nseg, j.lstm_hid = int(dgrad), dtype, Cout, Ctot, ks, stride, pad, len(segs), hid
    off = 0
    for i, c in enumerate(segs[:3]):
        j.Cseg[i] = c
        j.Coff[i] = offs[i] if offs is not None else off
        off += c
    j.imode = j.ldw = j.krows = -7                # a refused job keeps these
    blocks = L.rsis_conv_pack_job_fill(ctypes.byref(j))
    seg_arr = (ctypes.c_int * max(1, len(segs)))(*segs)
    return {"blocks": blocks, "imode": j.imode, "krows": j.krows, "ldw": j.ldw,
            "bytes_fwd": L.rsis_conv_packed_bytes_fwd(dtype, Cout, ks, stride, pad, len(segs), seg_arr),
            "bytes_dgrad": L.rsis_conv_packed_bytes_dgrad(dtype, Cout, ks, stride, pad, sum(segs))}


def record_all(L, PackJob):
    return {plan_id(case[0], dn, dgrad): record(L, PackJob, case, dt, dgrad) for case in CASES for dn, dt in DTYPES for dgrad in (0, 1)}
