"""The census of the Q15 serial-recurrence ladders: one entry per branch and per fall-back edge of the three places where the host picks between
hand-written bit-exact kernels by shape, alignment, stage count and environment switches --

  chain     the AudioFilterBiquad nodes behind a Q15 chain          msdr_chain_process         Chain.node_kernel()
  node      the stand-alone node                                    msdr_biquad_q15_update     BiquadQ15.last_kernel()
  frontend  DC block + amplifier + AGC()                            msdr_frontend_update       Frontend.last_kernel()

All of these kernels give the same bits, so a test that does not ask WHICH one ran proves nothing about the kernel its docstring names.
tests/test_gpu_q15_ladders.py runs every entry on the GPU, requires the getter to report `kernel` after every call and holds the output, the
state records and the memory around the buffer to the oracle; tests/test_q15_ladder_cases.py checks this table on the CPU.

`expected()` is written from the rules as include/msdr.h documents them (above msdr_chain_node_kernel) -- not from the library's code and
without importing anything of it: where the host and its documentation disagree, the census fails.

An entry:
  name, ladder, channels
  lengths      samples per call, three or more consecutive calls (state is carried)
  nodes        chain / node: stages per node -- () no node, (1,) one node of one stage, (1, 1) the reference's two nodes, (4, 1) Linkwitz-Riley
               four + notch
  env          switches set before the instance is created (every one is read at create time)
  align        bytes added to the 16-byte aligned data pointer (frontend: (input, output))
  per_channel  chain / node: per-channel records (set_coefficients_channels)
  pc_taps      chain: per-channel FIR taps (set_taps_channels); block_kernel: set_block_kernel_q15(1)
  fe_stages    frontend: "all" or "dc" (MSDR_FE_DCBLOCK alone); in_place: d_out == d_adc
  kernel       what the getter must report after every call
"""

CU_COUNT = 256           # MI355X; a partition has fewer.  No entry's expectation changes for any count from 8 to 256 (test_q15_ladder_cases.py)


def _e(name, ladder, channels, lengths, kernel, nodes=(), env=None, align=0, per_channel=False, pc_taps=False, block_kernel=False, fe_stages="all",
       in_place=False, note=""):
    if ladder == "frontend" and not isinstance(align, tuple):
        align = (align, align)
    return dict(name=name, ladder=ladder, channels=channels, lengths=tuple(lengths), kernel=kernel, nodes=tuple(nodes), env=dict(env or {}), align=align,
                per_channel=per_channel, pc_taps=pc_taps, block_kernel=block_kernel, fe_stages=fe_stages, in_place=in_place, note=note)


NO_FUSE = {"MSDR_Q15_NO_FUSE": "1"}
T128, T256, SLABS, RAGGED = (128, 128, 128), (256, 256, 256), (256, 384, 256), (130, 130, 130)
BLK, PC1, PC2, PIPE, LANE1, LANE2 = ("biquad_teensy_blk_kernel", "biquad_teensy_pc_kernel<1>", "biquad_teensy_pc_kernel<2>", "biquad_teensy_pipe_kernel",
                                     "biquad_teensy_kernel<1>", "biquad_teensy_kernel<2>")


def P4(nodes, ch):
    return "biquad_teensy_pipe4_kernel<%d,%d>" % (nodes, ch)


def FE4(ch):
    return "frontend_pipe4_kernel<%d>" % ch


ENTRIES = [
    # ---- the two nodes behind a chain (one stage each unless `nodes` says otherwise) ----------------------------------------------------------
    _e("c_fused", "chain", 48, T128, "chain_q15mb_kernel", (1, 1),
       note="the host fuses at this size without MSDR_MB_NW: among equal costs it prefers three waves per workgroup when the nodes can ride along"),
    _e("c_unfused", "chain", 48, T128, BLK, (1, 1), NO_FUSE),
    _e("c_blk_under_cu", "chain", 16, T128, BLK, (1, 1), NO_FUSE, note="1 workgroup <= any CU count"),
    _e("c_blk_over_cu", "chain", 4112, T128, P4(2, 16), (1, 1), NO_FUSE, note="16 x 257 channels: 257 workgroups > any CU count of this part"),
    _e("c_blk_on_over_cu", "chain", 4112, T128, BLK, (1, 1), dict(NO_FUSE, MSDR_BIQUAD_BLK="1")),
    _e("c_blk_off", "chain", 48, T128, P4(2, 16), (1, 1), dict(NO_FUSE, MSDR_BIQUAD_BLK="0")),
    _e("c_blk_on_n256", "chain", 48, T256, P4(2, 16), (1, 1), dict(NO_FUSE, MSDR_BIQUAD_BLK="1"), note="forced on, but not one 128-sample block"),
    _e("c_blk_on", "chain", 48, T128, BLK, (1, 1), dict(NO_FUSE, MSDR_BIQUAD_BLK="1")),
    _e("c_unfused_n256", "chain", 48, T256, P4(2, 16), (1, 1), NO_FUSE),
    _e("c_pipe4_16", "chain", 128, SLABS, P4(2, 16), (1, 1), {"MSDR_BIQUAD_PIPE_CH": "16"}),
    _e("c_pipe4_32", "chain", 128, SLABS, P4(2, 32), (1, 1), {"MSDR_BIQUAD_PIPE_CH": "32"}),
    _e("c_pipe4_64", "chain", 128, SLABS, P4(2, 64), (1, 1), {"MSDR_BIQUAD_PIPE_CH": "64"}),
    _e("c_pipe4_32_stream", "chain", 128, (128, 256, 384), P4(2, 32), (1, 1), {"MSDR_BIQUAD_PIPE_CH": "32", "MSDR_NO_BLOCK": "1", "MSDR_BIQUAD_BLK": "0"},
       note="a 128-sample call behind the streaming demodulator kernel"),
    _e("c_nodiv_32", "chain", 48, SLABS, LANE2, (1, 1), {"MSDR_BIQUAD_PIPE_CH": "32"}),
    _e("c_nodiv_64", "chain", 80, SLABS, LANE2, (1, 1), {"MSDR_BIQUAD_PIPE_CH": "64"}),
    _e("c_div_64", "chain", 128, SLABS, P4(2, 64), (1, 1), {"MSDR_BIQUAD_PIPE_CH": "64"}),
    _e("c_slabs_64", "chain", 64, T256, P4(2, 16), (1, 1)),
    _e("c_unaligned_2", "chain", 64, T256, LANE2, (1, 1), align=2),
    _e("c_unaligned_8", "chain", 64, T256, LANE2, (1, 1), align=8),
    _e("c_ragged", "chain", 64, RAGGED, LANE2, (1, 1)),
    _e("c_multi_slabs", "chain", 64, T256, PIPE, (4, 1)),
    _e("c_multi_80", "chain", 80, T256, LANE2, (4, 1)),
    _e("c_multi_unaligned", "chain", 64, T256, LANE2, (4, 1), align=2),
    _e("c_multi_ragged", "chain", 64, RAGGED, LANE2, (4, 1)),
    _e("c_multi_second_node", "chain", 64, T256, PIPE, (1, 2), note="the high-shelf + notch as node 1"),
    _e("c_per_channel", "chain", 48, T128, PC2, (1, 1), per_channel=True),
    _e("c_per_channel_ragged", "chain", 70, RAGGED, PC2, (1, 1), per_channel=True, align=2, note="any shape"),
    _e("c_pc_taps", "chain", 48, T128, PC2, (1, 1), per_channel=True, pc_taps=True),
    _e("c_block_kernel", "chain", 48, T128, "chain_q15pcb_kernel", (1, 1), per_channel=True, pc_taps=True, block_kernel=True),
    _e("c_one_node", "chain", 48, T128, P4(1, 16), (1,)),
    _e("c_one_node_70", "chain", 70, T128, LANE1, (1,)),
    _e("c_one_node_per_channel", "chain", 48, T128, PC1, (1,), per_channel=True),
    _e("c_no_nodes", "chain", 48, T128, "", ()),
    # ---- the stand-alone node ------------------------------------------------------------------------------------------------------------------
    _e("n_base", "node", 128, (128, 384, 128), P4(1, 16), (1,)),
    _e("n_16", "node", 16, (128, 384, 128), P4(1, 16), (1,)),
    _e("n_pipe4_16", "node", 128, (128, 384, 128), P4(1, 16), (1,), {"MSDR_BIQUAD_PIPE_CH": "16"}),
    _e("n_pipe4_32", "node", 128, (128, 384, 128), P4(1, 32), (1,), {"MSDR_BIQUAD_PIPE_CH": "32"}),
    _e("n_pipe4_64", "node", 128, (128, 384, 128), P4(1, 64), (1,), {"MSDR_BIQUAD_PIPE_CH": "64"}),
    _e("n_pipe4_32_one_group", "node", 32, (128, 384, 128), P4(1, 32), (1,), {"MSDR_BIQUAD_PIPE_CH": "32"}),
    _e("n_pipe4_64_one_group", "node", 64, (128, 384, 128), P4(1, 64), (1,), {"MSDR_BIQUAD_PIPE_CH": "64"}),
    _e("n_nodiv_32", "node", 48, (128, 384, 128), LANE1, (1,), {"MSDR_BIQUAD_PIPE_CH": "32"}),
    _e("n_nodiv_64", "node", 32, (128, 384, 128), LANE1, (1,), {"MSDR_BIQUAD_PIPE_CH": "64"}),
    _e("n_not_16", "node", 70, (128, 384, 128), LANE1, (1,)),
    _e("n_ragged", "node", 128, RAGGED, LANE1, (1,)),
    _e("n_unaligned_2", "node", 128, (128, 384, 128), LANE1, (1,), align=2),
    _e("n_unaligned_8", "node", 128, (128, 384, 128), LANE1, (1,), align=8),
    _e("n_two_stages", "node", 128, (128, 384, 128), LANE1, (2,)),
    _e("n_per_channel", "node", 128, (128, 384, 128), PC1, (1,), per_channel=True),
    # ---- the front end ---------------------------------------------------------------------------------------------------------------------------
    _e("f_base", "frontend", 128, (128, 256, 384), FE4(16)),
    _e("f_16", "frontend", 16, (128, 256, 384), FE4(16)),
    _e("f_pipe4_16", "frontend", 128, (128, 256, 384), FE4(16), env={"MSDR_FRONTEND_PIPE_CH": "16"}),
    _e("f_pipe4_32", "frontend", 128, (128, 256, 384), FE4(32), env={"MSDR_FRONTEND_PIPE_CH": "32"}),
    _e("f_pipe4_64", "frontend", 128, (128, 256, 384), FE4(64), env={"MSDR_FRONTEND_PIPE_CH": "64"}),
    _e("f_nodiv_32", "frontend", 48, (128, 256, 384), "frontend_kernel", env={"MSDR_FRONTEND_PIPE_CH": "32"}),
    _e("f_nodiv_64", "frontend", 96, (128, 256, 384), "frontend_kernel", env={"MSDR_FRONTEND_PIPE_CH": "64"}),
    _e("f_not_16", "frontend", 70, (128, 256, 384), "frontend_kernel"),
    _e("f_partial", "frontend", 128, (128, 256, 384), "frontend_kernel", fe_stages="dc"),
    _e("f_in_unaligned", "frontend", 128, (128, 256, 384), "frontend_kernel", align=(2, 0)),
    _e("f_out_unaligned", "frontend", 128, (128, 256, 384), "frontend_kernel", align=(0, 2)),
    _e("f_in_place", "frontend", 128, (128, 256, 384), FE4(16), in_place=True),
    _e("f_in_place_64", "frontend", 128, (128, 256, 384), FE4(64), env={"MSDR_FRONTEND_PIPE_CH": "64"}, in_place=True),
]
NAMES = [e["name"] for e in ENTRIES]
BY_NAME = {e["name"]: e for e in ENTRIES}

# Every condition of every ladder, with an entry on each side of it that differs from the other in `fields` only (and in the kernel).
#        ladder      condition                         one side            the other side          fields that may differ
EDGES = [("chain",    "fused / MSDR_Q15_NO_FUSE",       "c_fused",          "c_unfused",            ("env",)),
         ("chain",    "blk rule: CU count",             "c_blk_under_cu",   "c_blk_over_cu",        ("channels",)),
         ("chain",    "blk rule: forced on",            "c_blk_over_cu",    "c_blk_on_over_cu",     ("env",)),
         ("chain",    "blk rule: forced off",           "c_unfused",        "c_blk_off",            ("env",)),
         ("chain",    "n == 128 (blk forced on)",       "c_blk_on",         "c_blk_on_n256",        ("lengths",)),
         ("chain",    "n == 128 (host rule)",           "c_unfused",        "c_unfused_n256",       ("lengths",)),
         ("chain",    "channels % per_group (32)",      "c_pipe4_32",       "c_nodiv_32",           ("channels",)),
         ("chain",    "channels % per_group (64)",      "c_div_64",         "c_nodiv_64",           ("channels",)),
         ("chain",    "16-byte alignment (2)",          "c_slabs_64",       "c_unaligned_2",        ("align",)),
         ("chain",    "16-byte alignment (8)",          "c_slabs_64",       "c_unaligned_8",        ("align",)),
         ("chain",    "n % 128",                        "c_slabs_64",       "c_ragged",             ("lengths",)),
         ("chain",    "one stage or more",              "c_slabs_64",       "c_multi_slabs",        ("nodes",)),
         ("chain",    "one stage or more (node 1)",     "c_slabs_64",       "c_multi_second_node",  ("nodes",)),
         ("chain",    "channels % 64",                  "c_multi_slabs",    "c_multi_80",           ("channels",)),
         ("chain",    "16-byte alignment (pipe)",       "c_multi_slabs",    "c_multi_unaligned",    ("align",)),
         ("chain",    "n % 128 (pipe)",                 "c_multi_slabs",    "c_multi_ragged",       ("lengths",)),
         ("chain",    "per-channel records",            "c_fused",          "c_per_channel",        ("per_channel",)),
         ("chain",    "block kernel switch",            "c_pc_taps",        "c_block_kernel",       ("block_kernel",)),
         ("chain",    "one node or two",                "c_one_node",       "c_fused",              ("nodes",)),
         ("chain",    "no nodes",                       "c_no_nodes",       "c_one_node",           ("nodes",)),
         ("chain",    "one node: channels % per_group", "c_one_node",       "c_one_node_70",        ("channels",)),
         ("chain",    "one node: per-channel records",  "c_one_node",       "c_one_node_per_channel", ("per_channel",)),
         ("node",     "channels % per_group (32)",      "n_pipe4_32",       "n_nodiv_32",           ("channels",)),
         ("node",     "channels % per_group (64)",      "n_pipe4_64_one_group", "n_nodiv_64",       ("channels",)),
         ("node",     "channels % per_group (16)",      "n_base",           "n_not_16",             ("channels",)),
         ("node",     "n % 128",                        "n_base",           "n_ragged",             ("lengths",)),
         ("node",     "16-byte alignment (2)",          "n_base",           "n_unaligned_2",        ("align",)),
         ("node",     "16-byte alignment (8)",          "n_base",           "n_unaligned_8",        ("align",)),
         ("node",     "one stage or more",              "n_base",           "n_two_stages",         ("nodes",)),
         ("node",     "per-channel records",            "n_base",           "n_per_channel",        ("per_channel",)),
         ("frontend", "channels % per_group (32)",      "f_pipe4_32",       "f_nodiv_32",           ("channels",)),
         ("frontend", "channels % per_group (64)",      "f_pipe4_64",       "f_nodiv_64",           ("channels",)),
         ("frontend", "channels % per_group (16)",      "f_base",           "f_not_16",             ("channels",)),
         ("frontend", "all stages",                     "f_base",           "f_partial",            ("fe_stages",)),
         ("frontend", "16-byte alignment (input)",      "f_base",           "f_in_unaligned",       ("align",)),
         ("frontend", "16-byte alignment (output)",     "f_base",           "f_out_unaligned",      ("align",))]

# The conditions the issue of this census names, each of which must appear among EDGES for the ladders that have it
CONDITIONS = {"16-byte alignment": ("chain", "node", "frontend"), "n % 128": ("chain", "node"), "channels % per_group": ("chain", "node", "frontend"),
              "channels % 64": ("chain",), "one stage or more": ("chain", "node"), "per-channel records": ("chain", "node"), "n == 128": ("chain",),
              "blk rule": ("chain",)}

# Kernels of csrc/ named biquad_teensy* / frontend* that no call can reach, with the reason (none: frontend_pipe_kernel, the two-wave front-end
# pipeline, needed channels % 64 == 0 where one of the frontend_pipe4_kernel<16 | 32 | 64> launches had already been taken -- it was deleted)
UNREACHABLE = {}


def per_group(value, channels):
    """channels per workgroup of the slab pipelines, fixed at create time: the switch if it is 16 / 32 / 64, else by batch size"""
    if value in ("16", "32", "64"):
        return int(value)
    return 64 if channels >= 16384 else 32 if channels >= 8192 else 16


def _aligned(e, which=None):
    a = e["align"]
    return (a if which is None else a[which]) % 16 == 0


def expected_node(channels, n, stages, per_channel, aligned, env):
    """msdr_biquad_q15_last_kernel after an update() of n samples"""
    if per_channel:
        return PC1
    p = per_group(env.get("MSDR_BIQUAD_PIPE_CH"), channels)
    if stages == 1 and n % 128 == 0 and aligned and channels % p == 0:
        return P4(1, p)
    return LANE1


def expected(e, n, cu_count=CU_COUNT):
    """what the entry's getter reports after a call of n samples, by the rules of include/msdr.h"""
    ch, env = e["channels"], e["env"]
    if e["ladder"] == "node":
        return expected_node(ch, n, e["nodes"][0], e["per_channel"], _aligned(e), env)
    if e["ladder"] == "frontend":
        p = per_group(env.get("MSDR_FRONTEND_PIPE_CH"), ch)
        in_ok = _aligned(e, 0)
        out_ok = in_ok if e["in_place"] else _aligned(e, 1)
        if e["fe_stages"] == "all" and in_ok and out_ok and ch % p == 0:
            return FE4(p)
        return "frontend_kernel"
    nodes, aligned = e["nodes"], _aligned(e)
    if not nodes:
        return ""
    block_length = 32 <= n <= 512 and 1024 % n == 0
    if e["pc_taps"] and e["block_kernel"] and block_length:
        return "chain_q15pcb_kernel"
    if len(nodes) == 1:
        return expected_node(ch, n, nodes[0], e["per_channel"], aligned, env)
    one_stage = all(s == 1 for s in nodes)
    block_path = not e["pc_taps"] and block_length and aligned and "MSDR_NO_BLOCK" not in env          # info().kernel = chain_q15mb_kernel
    if block_path and one_stage and n == 128 and not e["per_channel"] and "MSDR_Q15_NO_FUSE" not in env and "MSDR_MB_NW" not in env and ch <= 16384:
        return "chain_q15mb_kernel"
    if e["per_channel"]:
        return PC2
    force = env.get("MSDR_BIQUAD_BLK")
    if one_stage and n == 128 and aligned and (force == "1" or (force is None and (ch + 15) // 16 <= cu_count)):
        return BLK
    p = per_group(env.get("MSDR_BIQUAD_PIPE_CH"), ch)
    if one_stage and n % 128 == 0 and aligned and ch % p == 0:
        return P4(2, p)
    if n % 128 == 0 and aligned and ch % 64 == 0:
        return PIPE
    return LANE2
