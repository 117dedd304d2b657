"""The arms of the A/B switches (docs/SWITCHES.md): one entry per non-default value that tools/ablation.sh times, as DATA -- no torch, no
package import: tests/test_switches.py reads this file and loads no library.

The timing of an arm means something only while the arm computes the right thing; an off arm is also the kernel the project falls back to
when a fusion is reverted.  Most switches are cached at import or at first use, so an arm cannot be reached by setting the variable inside
the pytest process: tests/switch_arm_child.py runs each arm -- and `default` -- in a process of its own, tests/test_hostsim_switch_arms.py
(emulator) and tests/test_gpu_switch_arms.py (GPU) start it and compare.

An arm:
  env      the variables of the arm (one switch, or the compound row of tools/ablation.sh)
  level    "cabi": read in csrc/ -- runs on the emulator and on the GPU; "ops" / "model": read in Python -- GPU only
  witness  {device: [(query, answer in a default process, answer in the arm's process)]}: proof that the arm was reached.  Both answers are
           asserted, each in a fresh process.  A device without one says why under `unseen` and relies on the other device's.
  cases    {device: [case]}: what must hold under the arm, through the shared case bodies at THEIR bounds (no case has a tolerance of its own)
           -- every geometry of the existing lists whose witness query changes under the arm, geometries no list had, and neighbours whose
           dispatch the arm leaves alone.  At most 8 on the emulator (a convolution case costs ~1.4 s there).

Queries (tests/switch_arm_child.py `answer`):
  ("conv_describe", geometry, direction)            hifihr_conv2d_describe
  ("bgemm_describe", tn, (M, N, K, batch)[, route]) hifihr_bgemm_describe_batch          route: a name of kernel_cases.GEMM_ROUTES, applied on
                                                    the emulator only (its 4 compute units; the GPU runs every query and case on its own 256)
  ("pred", method, args[, route])                   a predicate / count of hifihr_amd._lib.HifihrLib
  ("launched", kind, args, substring[, route])      emulator: a kernel whose logged name contains `substring` ran in the call
  ("profiled", kind, args, substring)               GPU: the same, from the kernel names torch's profiler reports
  ("tn_skip", (N, H, W, C, K)[, route])             which rows hifihr_wino_wgrad_gemm_parts sums when finite non-zero values stand behind the
                                                    last computed tile of a mosaic: "valid" / "all" (with zeros there -- the cases -- both agree)
  ("conv_log", case, log)                           the dispatch case passes with exactly this ops.PROFILE.conv_log
  ("events", case, log, name)                       a launch bracketed `name` (ops.PROFILE.events) ran in the dispatch case
  ("calls", case, log, entry)                       the C-ABI entry was called in the dispatch case
  ("early", case, log)                              ops._DEFER_DW flushed early, beside the stem's backward, in the dispatch case
  ("model", key, ...)                               of the third training step of BASELINE configs[1] at batch 4: entries called, branches, ...

Cases (`run_case`): ("conv", geometry) conv_contract_case (+ on the emulator describe against the launch log); ("pair", pair[, route])
conv_pair_contract_case; ("nt" / "tn", shape) bgemm_*_contract_case; ("wino", layer + (m,)[, route]) wino_chain_contract_case; ("wino_bn", g);
("render", case); ("dispatch", name, log) tests/test_gpu_conv.py _run_dispatch_case with the log written here -- a case of its `_cases`, or one of the
child's own, which go the way hifihr_amd/network.py goes (through the predicate the arm turns off, then the fallback): stem_block,
defer_chain (stem block -> 64 -> 64 layer, beside an F(4x4) layer: every deferred weight gradient against float64), bn_block, pair_block;
("model", "losses" | "chain") the bodies of test_train_step_losses_match_oracle / test_backward_chain_matches_oracle_from_features.

A log is [(tag, direction)]; tags name the geometries tests/test_gpu_conv.py `_geoms` picks in the DEFAULT process (the arms get the same
ones): f4 / f4T the F(4x4) layer and its transpose (f4m2 / f4Tm2: at F(2x2)), f4d the same layer on the direct kernels, f2 / f2T / f2d the
F(2x2) layer, gc the 64 -> 64 layer, gs / gs1 the strided 3x3 and its 1x1 twin, pair their forward pair, p1 the 1x1 producer of the
batch-norm case, gst the stem, gsb the stem block, gsc the stem in front of gc (defer_chain)."""

# ---- logs of the dispatch cases -----------------------------------------------------------------------------------------------------------
F4_PAIRED = [("f4", "gemm"), ("f4", "gemm-pair")]
F4_APART = [("f4", "gemm"), ("f4T", "gemm"), ("f4", "gemm-tn")]
F4_M2 = [("f4m2", "gemm"), ("f4Tm2", "gemm"), ("f4m2", "gemm-tn")]
direct = lambda g: [(g, "fwd"), (g, "dgrad"), (g, "wgrad")]
C64_PAIR = [("gc", "fwd-wino2"), ("gc", "c64-pair")]
C64_APART = [("gc", "fwd-wino2"), ("gc", "dgrad-wino2"), ("gc", "wgrad")]
C64_PLAIN = [("gc", "fwd-wino2"), ("gc", "dgrad-wino2")]
BN_P1 = [("p1", "fwd"), ("p1", "dgrad")]
PAIR_BOTH = [("pair", "fwd-pair"), ("gs", "dgrad+1x1"), ("gs", "wgrad+1x1")]
PAIR_W_APART = [("pair", "fwd-pair"), ("gs", "dgrad+1x1"), ("gs", "wgrad"), ("gs1", "wgrad")]
PAIR_FALLBACK = [("pair", "fwd-pair"), ("gs", "dgrad"), ("gs", "wgrad"), ("gs1", "dgrad"), ("gs1", "wgrad")]
STEM = [("gst", "fwd"), ("gst", "wgrad")]
STEM_BLOCK = [("gsb", "fwd"), ("gsb", "wgrad")]
DEFER_CHAIN = [("gsc", "fwd"), ("gsc", "wgrad")] + C64_PAIR + F4_PAIRED
PAIR_APART = direct("gs") + direct("gs1")          # network.BasicBlock without the pair launch (the 1x1's data gradient goes through the fork)

# ---- geometries ---------------------------------------------------------------------------------------------------------------------------
S2 = (1, 7, 7, 32, 128, 3, 3, 2, 1)               # the gathering row-share forward
S2_GPU = (8, 28, 28, 64, 128, 3, 3, 2, 1)
HALO, HALO_RAGGED, HALO_GPU = (1, 3, 14, 64, 64, 3, 3, 1, 1), (1, 5, 15, 64, 64, 3, 3, 1, 1), (16, 56, 56, 64, 64, 3, 3, 1, 1)
STEM7, STEM7_GPU = (1, 4, 56, 4, 64, 7, 7, 2, 3), (8, 56, 56, 4, 64, 7, 7, 2, 3)
G1X1, G1X1_GPU = (1, 4, 4, 256, 128, 1, 1, 1, 0), (32, 14, 14, 256, 128, 1, 1, 1, 0)
PLUS = (1, 12, 12, 32, 64, 3, 3, 2, 1)            # both plus1x1 backward launches
PAIR0, PAIR_GPU = (2, 12, 12, 32, 2, 128, 3, 1, 128, 1, 0), (16, 28, 28, 64, 2, 128, 3, 1, 128, 1, 0)
# HIFIHR_CONV_ROWS=2: 3x3 at strides 1, 3, 4 (pads below, at and above the filter's), 1x1 at strides 2 and 4 with pad 0 and a pad >= the filter
ROWS2_NEW = [(1, 7, 6, 32, 128, 3, 3, 1, 1), (1, 9, 11, 64, 128, 3, 3, 3, 1), (1, 6, 5, 32, 128, 1, 1, 4, 2), (1, 5, 6, 32, 128, 3, 3, 1, 3),
             (2, 5, 4, 32, 128, 3, 3, 4, 0), (2, 5, 4, 32, 128, 1, 1, 4, 0)]
ROWS2_SAME = [(2, 7, 5, 32, 128, 1, 1, 2, 0), (1, 6, 5, 32, 128, 1, 1, 2, 1)]          # stride 2: on the row-share kernel already
ROWS2_GPU = (5, 31, 29, 32, 128, 3, 3, 1, 1)      # 4 495 rows: more than 256 shares of 16
MOSAIC_TN, MOSAIC_TN_GPU = (16, 5, 5, 128, 128), (32, 14, 14, 256, 256)      # mosaic layers whose weight-gradient product runs on bgemm_tn_rows_kernel
ROWS, IGEMM = "bgemm_nt_rows_kernel<2>", "conv_igemm_kernel"
TN_ROWS, TN_TILE, NT_ROWS, NT_TILE = "bgemm_tn_rows_kernel", "bgemm_tn_kernel<64, 64>", "bgemm_nt_rows_kernel<0>", "bgemm_nt_kernel<64, 64>"

conv = lambda *gs: [("conv", g) for g in gs]
nt = lambda *gs: [("nt", g + ("default", "full")) for g in gs]
tn = lambda *gs: [("tn", (g + ("default",)) if len(g) == 4 else g) for g in gs]
wino = lambda *gs: [("wino", g[:5] + (4,), "cus16" if g[3:5] == (128, 128) else None) for g in gs]
disp = lambda **kw: [("dispatch", k, v) for k, v in kw.items()]
MODEL = [("model", "losses"), ("model", "chain")]


def _arm(env, level, witness, cases, unseen=None):
    return {"env": {k: str(v) for k, v in env.items()}, "level": level, "witness": witness, "cases": cases, "unseen": unseen or {}}


ARMS = {"default": _arm({}, "cabi", {"cpu": [], "cuda": []}, {"cpu": conv(S2) + tn((128, 128, 64, 16)), "cuda": conv(S2) + disp(f4=F4_PAIRED)})}

# ---- csrc/gemm.hip ------------------------------------------------------------------------------------------------------------------------
ARMS["gemm_rows_0"] = _arm(
    {"HIFIHR_GEMM_ROWS": 0}, "cabi",
    {d: [(("bgemm_describe", 0, (17, 128, 32, 2)), NT_ROWS, NT_TILE), (("bgemm_describe", 0, (300, 576, 128, 1)), "bgemm_nt_rows_kernel<1>", NT_TILE),
         (("conv_describe", S2, 0), ROWS, IGEMM)] for d in ("cpu", "cuda")},
    {"cpu": nt((15, 128, 32, 2), (128, 256, 64, 1), (65, 256, 512, 1), (300, 576, 128, 1), (1, 128, 512, 5), (64, 64, 160, 1), (17, 192, 96, 2)) + conv(S2),
     # (without the row-share NT kernel the paired F(4x4) backward has no NT half: two products)
     "cuda": nt((15, 128, 32, 2), (128, 256, 64, 1), (65, 256, 512, 1), (300, 576, 128, 1), (300, 256, 96, 2), (64, 64, 160, 1), (17, 192, 96, 2))
     + conv(S2, S2_GPU) + disp(f4=F4_APART, direct_pre_stats=direct("gs"))})
ARMS["gemm_tn_rows_0"] = _arm(
    {"HIFIHR_GEMM_TN_ROWS": 0}, "cabi",
    {"cpu": [(("bgemm_describe", 1, (128, 128, 64, 16)), TN_ROWS, TN_TILE), (("bgemm_describe", 1, (128, 128, 256, 2)), TN_ROWS, TN_TILE)],
     "cuda": [(("bgemm_describe", 1, (128, 128, 1024, 36)), TN_ROWS, TN_TILE), (("conv_log", "f4", F4_PAIRED), sorted("%s:%s" % e for e in F4_PAIRED), None)]},
    {"cpu": tn((128, 128, 64, 16), (320, 128, 96, 2), (192, 256, 96, 2), (128, 128, 256, 2), (256, 128, 64, 16, "cus16"), (64, 64, 32, 36), (128, 64, 31, 1))
     + wino(MOSAIC_TN),
     "cuda": tn((128, 128, 1024, 36), (256, 256, 1024, 36), (128, 128, 64, 16), (64, 64, 32, 36)) + wino(MOSAIC_TN_GPU) + disp(f4=F4_APART)})
ARMS["gemm_tn_split_0"] = _arm(
    {"HIFIHR_GEMM_TN_SPLIT": 0}, "cabi",
    # (128, 128, 256, 2) on the emulator's 4 compute units: too few blocks for complete products, 8 chunks -- two slabs of the row-share
    # kernel, without the split one slab of the per-tile kernel; on 256 compute units (128, 128, 1024, 36): 8 slabs, then 4 of 64x64 tiles
    {"cpu": [(("pred", "bgemm_tn_parts", (128, 128, 256, 2)), 2, 1), (("bgemm_describe", 1, (128, 128, 256, 2)), TN_ROWS, TN_TILE)],
     "cuda": [(("pred", "bgemm_tn_parts", (128, 128, 1024, 36)), 8, 4), (("bgemm_describe", 1, (128, 128, 1024, 36)), TN_ROWS, TN_TILE)]},
    # (no Winograd layer of the lists splits on 4 compute units: a 128-channel layer has 288 blocks, complete products)
    {"cpu": tn((128, 128, 256, 2), (128, 128, 64, 16), (128, 128, 32, 2), (320, 128, 96, 2)),
     "cuda": tn((128, 128, 1024, 36), (256, 256, 1024, 36), (128, 128, 64, 16)) + wino(MOSAIC_TN_GPU) + disp(f4=F4_APART)})
ARMS["gemm_tn_coherent_0"] = _arm(
    {"HIFIHR_GEMM_TN_COHERENT": 0}, "cabi",
    # the schedule changes the order in which workgroups take tiles: same kernel name, same slab count, the same bits -- the only thing
    # that tells the arms apart is hifihr_bgemm_tn_coherent, the BgemmArgs::co_r of the launch (problems an XCD owns per round; 0:
    # contiguous shares).  It needs a multiple of 8 workgroups: 16 on the emulator; on 256 compute units an XCD's 32 workgroups want 8
    # whole tiles each per round, which the 1024-row products of the lists above do not give (their operands would not fit an L2).
    {"cpu": [(("pred", "bgemm_tn_coherent", (256, 128, 64, 16), "cus16"), 1, 0), (("pred", "bgemm_tn_coherent", (256, 128, 64, 20), "cus16"), 1, 0),
             (("pred", "bgemm_tn_coherent", (128, 128, 64, 16), "cus16"), 0, 0)],
     "cuda": [(("pred", "bgemm_tn_coherent", (512, 512, 128, 36)), 2, 0), (("pred", "bgemm_tn_coherent", (256, 256, 256, 36)), 8, 0),
              (("pred", "bgemm_tn_coherent", (128, 128, 1024, 36)), 0, 0)]},
    {"cpu": tn((256, 128, 64, 16, "cus16"), (256, 128, 64, 20, "cus16"), (128, 128, 64, 16, "cus16"), (320, 128, 96, 2)),
     "cuda": tn((512, 512, 128, 36), (256, 256, 256, 36), (128, 128, 1024, 36), (128, 128, 64, 16))})
ARMS["gemm_tn_skip_0"] = _arm(
    {"HIFIHR_GEMM_TN_SKIP": 0}, "cabi",
    {"cpu": [(("tn_skip", MOSAIC_TN, "cus16"), "valid", "all")], "cuda": [(("tn_skip", MOSAIC_TN_GPU), "valid", "all")]},
    {"cpu": wino(MOSAIC_TN, (16, 5, 5, 4, 4), (1, 4, 4, 64, 64)), "cuda": wino(MOSAIC_TN_GPU, MOSAIC_TN, (16, 6, 6, 64, 64))})
ARMS["gemm_pair_0"] = _arm(
    {"HIFIHR_GEMM_PAIR": 0}, "cabi",
    {"cpu": [(("pred", "wino4_bwd_gemm_pair_supported", MOSAIC_TN, "cus16"), True, False)],
     "cuda": [(("pred", "wino4_bwd_gemm_pair_supported", (32, 28, 28, 128, 128)), True, False),
              (("conv_log", "f4", F4_PAIRED), sorted("%s:%s" % e for e in F4_PAIRED), None)]},
    {"cpu": wino(MOSAIC_TN, (2, 7, 5, 128, 64), (1, 4, 4, 64, 64)),
     "cuda": wino(MOSAIC_TN_GPU, MOSAIC_TN) + disp(f4=F4_APART, f4_async=F4_APART, f4_bias_relu=F4_APART, f4_unprepared=F4_APART, bn_wino_fused=BN_P1 + F4_APART)})
ARMS["conv_rows_0"] = _arm(
    {"HIFIHR_CONV_ROWS": 0}, "cabi",
    {"cpu": [(("conv_describe", S2, 0), ROWS, IGEMM), (("pred", "conv2d_fwd_bnstats_pair_supported", PAIR0, "cus16"), True, False)],
     "cuda": [(("conv_describe", S2, 0), ROWS, IGEMM), (("conv_describe", S2_GPU, 0), ROWS, IGEMM), (("pred", "conv2d_fwd_bnstats_pair_supported", PAIR_GPU), True, False),
              (("conv_log", "pair_block", PAIR_BOTH), sorted("%s:%s" % e for e in PAIR_BOTH), None)]},
    {"cpu": conv(S2, ROWS2_SAME[0], (1, 10, 9, 32, 64, 3, 3, 2, 1), (1, 11, 10, 32, 48, 3, 3, 3, 1)) + [("pair", PAIR0, "cus16")],
     "cuda": conv(S2, S2_GPU, ROWS2_SAME[0], (1, 10, 9, 32, 64, 3, 3, 2, 1), (1, 11, 10, 32, 48, 3, 3, 3, 1)) + [("pair", PAIR_GPU)]
     + disp(direct_pre_stats=direct("gs"), direct_pre_res=direct("gs"), pair_block=PAIR_APART)})
ARMS["conv_rows_2"] = _arm(
    {"HIFIHR_CONV_ROWS": 2}, "cabi",
    {d: [(("conv_describe", g, 0), IGEMM, ROWS) for g in ROWS2_NEW] + [(("conv_describe", g, 0), ROWS, ROWS) for g in ROWS2_SAME]
        + ([(("conv_describe", ROWS2_GPU, 0), IGEMM, ROWS)] if d == "cuda" else []) for d in ("cpu", "cuda")},
    {"cpu": conv(*ROWS2_NEW, *ROWS2_SAME), "cuda": conv(*ROWS2_NEW, *ROWS2_SAME, ROWS2_GPU, S2_GPU)})
ARMS["conv_rows_pair_0"] = _arm(
    {"HIFIHR_CONV_ROWS_PAIR": 0}, "cabi",
    {"cpu": [(("pred", "conv2d_fwd_bnstats_pair_supported", PAIR0, "cus16"), True, False), (("conv_describe", S2, 0), ROWS, ROWS)],
     "cuda": [(("pred", "conv2d_fwd_bnstats_pair_supported", PAIR_GPU), True, False), (("conv_describe", S2_GPU, 0), ROWS, ROWS),
              (("conv_log", "pair_block", PAIR_BOTH), sorted("%s:%s" % e for e in PAIR_BOTH), None)]},
    # (ops.conv2d_pair calls the pair entry whatever the switch says -- only hifihr_amd/network.py asks ops.conv2d_pair_ok -- so the dispatch
    #  cases `pair_*` of tests/test_gpu_conv.py cannot run here; pair_block asks, as the network does: the fwd-pair entry becomes two fwd)
    {"cpu": [("pair", PAIR0, "cus16"), ("pair", (1, 9, 11, 64, 2, 128, 3, 0, 256, 1, 0), "cus16"), ("pair", (1, 10, 9, 32, 2, 128, 1, 1, 128, 3, 2), "cus16"),
             ("pair", (1, 7, 7, 32, 2, 128, 3, 2, 128, 3, 0), "cus16"), ("pair", (1, 8, 8, 32, 1, 128, 3, 1, 128, 1, 0), "cus16"),
             ("pair", (1, 8, 8, 32, 2, 128, 5, 2, 128, 1, 0), "cus16")] + conv(S2),
     "cuda": [("pair", PAIR_GPU), ("pair", (8, 29, 27, 32, 2, 128, 3, 0, 256, 1, 0)), ("pair", (1, 8, 8, 32, 1, 128, 3, 1, 128, 1, 0))] + conv(S2, S2_GPU)
     + disp(direct_pre_stats=direct("gs"), pair_block=PAIR_APART)})

# ---- csrc/conv.hip, csrc/hifihr_api.hip, csrc/conv_halo.hip ---------------------------------------------------------------------------------
_1X1 = [(("conv_describe", G1X1, 0), NT_ROWS, IGEMM), (("conv_describe", G1X1, 1), NT_ROWS, IGEMM)]
_1X1_CASES = conv(G1X1, (1, 4, 6, 136, 232, 1, 1, 1, 0), (2, 3, 5, 64, 128, 1, 1, 1, 0), (2, 7, 5, 32, 48, 1, 1, 2, 0), (2, 7, 9, 32, 64, 2, 2, 1, 0))
ARMS["conv1x1_gemm_0"] = _arm({"HIFIHR_CONV1X1_GEMM": 0}, "cabi", {"cpu": _1X1, "cuda": _1X1 + [(("conv_describe", G1X1_GPU, 0), NT_ROWS, IGEMM)]},
                              {"cpu": _1X1_CASES, "cuda": _1X1_CASES + conv(G1X1_GPU) + disp(bn_wino_fused=BN_P1 + F4_PAIRED)})
_BOTH = [(("bgemm_describe", 0, (17, 128, 32, 2)), NT_ROWS, NT_TILE), (("conv_describe", S2, 0), ROWS, IGEMM)] + _1X1
ARMS["gemm_rows_0_conv1x1_gemm_0"] = _arm({"HIFIHR_GEMM_ROWS": 0, "HIFIHR_CONV1X1_GEMM": 0}, "cabi", {"cpu": _BOTH, "cuda": _BOTH},
                                          {"cpu": conv(G1X1, (1, 4, 6, 136, 232, 1, 1, 1, 0), S2) + nt((128, 256, 64, 1), (300, 576, 128, 1)),
                                           "cuda": conv(G1X1, (1, 4, 6, 136, 232, 1, 1, 1, 0), S2, G1X1_GPU, S2_GPU) + nt((128, 256, 64, 1), (300, 576, 128, 1))})
_PLUS_CASES = conv(PLUS, (1, 9, 13, 16, 32, 3, 3, 2, 1), (1, 10, 9, 32, 64, 3, 3, 2, 1), S2, (1, 11, 10, 32, 48, 3, 3, 3, 1), (1, 9, 8, 12, 20, 3, 3, 1, 1))
ARMS["wgrad_plus1x1_0"] = _arm(
    {"HIFIHR_WGRAD_PLUS1X1": 0}, "cabi",
    {"cpu": [(("pred", "conv2d_bwd_weight_plus1x1_supported", PLUS), True, False)],
     "cuda": [(("pred", "conv2d_bwd_weight_plus1x1_supported", PLUS), True, False), (("pred", "conv2d_bwd_weight_plus1x1_supported", S2_GPU), True, False),
              (("conv_log", "pair_both_wgrads", PAIR_BOTH), sorted("%s:%s" % e for e in PAIR_BOTH), None)]},
    {"cpu": _PLUS_CASES, "cuda": _PLUS_CASES + conv(S2_GPU) + disp(pair_both_wgrads=PAIR_W_APART, pair_w_apart=PAIR_W_APART)})
ARMS["dgrad_plus1x1_0"] = _arm(
    {"HIFIHR_DGRAD_PLUS1X1": 0}, "cabi",
    {"cpu": [(("pred", "conv2d_bwd_data_pre_plus1x1_supported", PLUS), True, False)],
     "cuda": [(("pred", "conv2d_bwd_data_pre_plus1x1_supported", PLUS), True, False), (("pred", "conv2d_bwd_data_pre_plus1x1_supported", S2_GPU), True, False),
              (("conv_log", "pair_both_wgrads", PAIR_BOTH), sorted("%s:%s" % e for e in PAIR_BOTH), None)]},
    # (without the tap the 1x1 twin's data gradient is a launch of its own and comes back in as the fork residual; the two weight
    #  gradients then run apart as well: ops._Conv2dPair.backward fuses them only behind the fused data gradient)
    {"cpu": _PLUS_CASES, "cuda": _PLUS_CASES + conv(S2_GPU) + disp(pair_both_wgrads=PAIR_FALLBACK, pair_w_apart=PAIR_FALLBACK)})
_HALO_CASES = conv(HALO, HALO_RAGGED, (1, 6, 5, 32, 4, 3, 3, 1, 1), (1, 9, 8, 12, 20, 3, 3, 1, 1))
# (the one-launch backward of a 64 -> 64 layer needs the halo weight gradient: without it the data gradient and the weight gradient run apart)
_HALO_DISP = disp(c64_pair_deferred=C64_APART, c64_pair_immediate=C64_APART, c64_res=C64_PLAIN, direct_unprepared_fork=direct("gc"))
ARMS["conv_halo_0"] = _arm(
    {"HIFIHR_CONV_HALO": 0}, "cabi",
    {d: [(("conv_describe", HALO, 0), "conv_halo_kernel", IGEMM), (("conv_describe", HALO, 1), "conv_halo_kernel", IGEMM),
         (("conv_describe", HALO, 2), "conv_halo_wgrad_kernel", "conv_wgrad_kernel"), (("conv_describe", HALO_RAGGED, 0), "conv_halo_kernel", IGEMM)]
        + ([(("conv_describe", HALO_GPU, 0), "conv_halo_kernel", IGEMM)] if d == "cuda" else []) for d in ("cpu", "cuda")},
    {"cpu": _HALO_CASES, "cuda": _HALO_CASES + conv(HALO_GPU) + _HALO_DISP})
ARMS["conv_halo_wgrad_0"] = _arm(
    {"HIFIHR_CONV_HALO_WGRAD": 0}, "cabi",
    {d: [(("conv_describe", HALO, 2), "conv_halo_wgrad_kernel", "conv_wgrad_kernel"), (("conv_describe", HALO, 0), "conv_halo_kernel", "conv_halo_kernel")]
        + ([(("conv_describe", HALO_GPU, 2), "conv_halo_wgrad_kernel", "conv_wgrad_kernel")] if d == "cuda" else []) for d in ("cpu", "cuda")},
    {"cpu": _HALO_CASES, "cuda": _HALO_CASES + conv(HALO_GPU) + _HALO_DISP})
_STEM_CASES = conv(STEM7, (1, 9, 9, 4, 64, 7, 7, 2, 3), (1, 9, 8, 16, 16, 7, 7, 1, 0))
ARMS["conv_stem_0"] = _arm(
    {"HIFIHR_CONV_STEM": 0}, "cabi",
    {d: [(("conv_describe", STEM7, 0), "conv_stem_kernel", IGEMM), (("conv_describe", STEM7, 2), "conv_stem_wgrad_kernel", "conv_wgrad_kernel")]
        + ([(("conv_describe", STEM7_GPU, 0), "conv_stem_kernel", IGEMM)] if d == "cuda" else []) for d in ("cpu", "cuda")},
    {"cpu": _STEM_CASES, "cuda": _STEM_CASES + conv(STEM7_GPU) + disp(stem_c3=STEM, stem_c3_unprepared=STEM)})
_GC = (4, 28, 28, 64, 64)
ARMS["conv_wino2_0"] = _arm(
    {"HIFIHR_CONV_WINO2": 0}, "cabi",
    {"cpu": [(("pred", "conv3x3_c64_wino_supported", _GC), True, False)],
     "cuda": [(("pred", "conv3x3_c64_wino_supported", _GC), True, False), (("conv_log", "c64_pair_deferred", C64_PAIR), sorted("%s:%s" % e for e in C64_PAIR), None)]},
    {"cpu": conv(HALO),                         # (the plain entries of a 64 -> 64 layer: the halo kernels the arm falls back to)
     "cuda": conv(HALO, HALO_GPU) + disp(c64_pair_deferred=direct("gc"), c64_res=direct("gc")[:2], direct_wgrad_slabs=[("gc", "fwd"), ("gc", "wgrad")],
                                         direct_unprepared_fork=direct("gc"))})
ARMS["c64_pair_0"] = _arm(
    {"HIFIHR_C64_PAIR": 0}, "ops",
    {"cuda": [(("pred", "conv3x3_c64_bwd_pair_supported", (4, 28, 28)), True, False),
              (("conv_log", "c64_pair_deferred", C64_PAIR), sorted("%s:%s" % e for e in C64_PAIR), None)]},
    {"cuda": disp(c64_pair_deferred=C64_APART, c64_pair_immediate=C64_APART, c64_pair_async=C64_APART, c64_res=C64_PLAIN)})

# ---- csrc/wino4.hip, the Winograd choices ----------------------------------------------------------------------------------------------------
_MOSAIC_W = [(("pred", "wino_tiles_computed", (16, 5, 5, 4)), 36, 64), (("pred", "wino_tiles_computed", (16, 6, 6, 4)), 49, 64),
             (("pred", "wino_tiles_computed", (17, 5, 5, 4)), 68, 68)]
_MOSAIC_C = (wino((16, 5, 5, 4, 4), (16, 6, 6, 64, 64), MOSAIC_TN, (32, 5, 5, 4, 4), (17, 5, 5, 4, 8), (16, 5, 6, 4, 4))
             + [("wino_bn", (16, 5, 5, 64, 4, True, False)), ("wino_bn", (16, 6, 6, 4, 4, False, False))])
ARMS["wino_mosaic_0"] = _arm({"HIFIHR_WINO_MOSAIC": 0}, "cabi",
                             {"cpu": _MOSAIC_W, "cuda": _MOSAIC_W + [(("pred", "wino_tiles_computed", (32, 14, 14, 4)), 450, 512)]},
                             {"cpu": _MOSAIC_C, "cuda": _MOSAIC_C + wino(MOSAIC_TN_GPU)})
_DW_C = wino((1, 4, 4, 64, 64), (2, 7, 5, 128, 64), (3, 9, 9, 8, 24), (1, 5, 6, 100, 8), (1, 4, 4, 176, 192))      # (the last: K C / 4 > 8192, narrow in both)
ARMS["wino_dw_wide_0"] = _arm(
    {"HIFIHR_WINO_DW_WIDE": 0}, "cabi",
    {"cpu": [(("launched", "dw_parts", (64, 64), "parts_wide_kernel"), True, False), (("launched", "dw_parts", (176, 192), "parts_wide_kernel"), False, False)],
     "cuda": [(("profiled", "dw_parts", (64, 64), "parts_wide_kernel"), True, False), (("profiled", "dw_parts", (176, 192), "parts_wide_kernel"), False, False)]},
    {"cpu": _DW_C, "cuda": _DW_C})
ARMS["wino_m_2"] = _arm(
    {"HIFIHR_WINO_M": 2}, "cabi",
    {"cpu": [(("pred", "wino_tile", (2, 7, 5, 128, 128)), 4, 2)],
     "cuda": [(("pred", "wino_tile", (32, 28, 28, 128, 128)), 4, 2), (("conv_log", "f4", F4_PAIRED), sorted("%s:%s" % e for e in F4_PAIRED), None)]},
    {"cpu": [("wino", (2, 7, 5, 128, 64, 2)), ("wino", (2, 7, 5, 128, 64, 4)), ("wino", (1, 4, 4, 64, 64, 2))],
     "cuda": [("wino", (2, 7, 5, 128, 64, 2)), ("wino", (16, 6, 6, 64, 64, 2))] + disp(f4=F4_M2, f4_bias_relu=F4_M2, f4_mask_in_output_transform=F4_M2, f4_unprepared=F4_M2)})
ARMS["winograd_0"] = _arm(
    {"HIFIHR_WINOGRAD": 0}, "ops",
    {"cuda": [(("conv_log", "f4", F4_PAIRED), sorted("%s:%s" % e for e in F4_PAIRED), None),
              (("conv_log", "c64_pair_deferred", C64_PAIR), sorted("%s:%s" % e for e in C64_PAIR), None)]},
    {"cuda": disp(f4=direct("f4d"), f4_bias_relu=direct("f4d"), f2_atomic=direct("f2d"), c64_pair_deferred=direct("gc"), c64_res=direct("gc")[:2])})

# ---- ops.py -------------------------------------------------------------------------------------------------------------------------------
_FUSED = BN_P1 + F4_PAIRED
ARMS["bn_wino_bwd_0"] = _arm({"HIFIHR_BN_WINO_BWD": 0}, "ops", {"cuda": [(("calls", "bn_wino_fused", _FUSED, "wino_output_transform_bnred"), True, False)]},
                             {"cuda": disp(bn_wino_fused=_FUSED, bn_wino_fused_to_autograd=_FUSED)})
# The three arms below change nothing in `chain` (it runs the encoder under no_grad and opens no prepared_weights scope), and `losses`
# bounds the forward alone: what they change in BACKWARD is held by a dispatch case of the child's own, against float64 autograd.
ARMS["bn_wino_fuse_0"] = _arm({"HIFIHR_BN_WINO_FUSE": 0}, "model",
                              {"cuda": [(("calls", "bn_block", _FUSED, "wino_bn_input_transform"), True, False), (("model", "calls", "wino_bn_input_transform"), True, False)]},
                              {"cuda": disp(bn_block=_FUSED) + MODEL[:1]})
ARMS["bn_pool_0"] = _arm({"HIFIHR_BN_POOL": 0}, "ops",
                         {"cuda": [(("events", "stem_block", STEM_BLOCK, "bn_pool_fwd"), True, False), (("events", "stem_block", STEM_BLOCK, "maxpool_fwd"), False, True)]},
                         {"cuda": disp(stem_block=STEM_BLOCK)})
ARMS["stem_reduce_y_0"] = _arm({"HIFIHR_STEM_REDUCE_Y": 0}, "ops",
                               {"cuda": [(("calls", "stem_block", STEM_BLOCK, "bn_relu_maxpool_bwd_y"), True, False),
                                         (("calls", "stem_block", STEM_BLOCK, "bn_relu_maxpool_bwd"), False, True)]},
                               {"cuda": disp(stem_block=STEM_BLOCK)})
ARMS["defer_dw_0"] = _arm({"HIFIHR_DEFER_DW": 0}, "model",
                          {"cuda": [(("calls", "f4", F4_PAIRED, "wino4_dw_transform_multi"), True, False), (("calls", "f4", F4_PAIRED, "wino_dw_transform_parts"), False, True),
                                    (("calls", "defer_chain", DEFER_CHAIN, "conv_halo_wgrad_reduce_multi"), True, False),
                                    (("model", "calls", "wino4_dw_transform_multi"), True, False)]},
                          {"cuda": disp(f4=F4_PAIRED, c64_pair_deferred=C64_PAIR, bn_wino_fused=_FUSED, defer_chain=DEFER_CHAIN) + MODEL[:1]})
ARMS["defer_early_0"] = _arm({"HIFIHR_DEFER_EARLY": 0}, "model",
                             {"cuda": [(("early", "defer_chain", DEFER_CHAIN), True, False), (("calls", "defer_chain", DEFER_CHAIN, "wino4_dw_transform_multi"), True, True),
                                       (("model", "n_early"), True, False), (("model", "calls", "wino4_dw_transform_multi"), True, True)]},
                             {"cuda": disp(defer_chain=DEFER_CHAIN) + MODEL[:1]})

# ---- models.py, losses.py -------------------------------------------------------------------------------------------------------------------
ARMS["light_branch_0"] = _arm({"HIFIHR_LIGHT_BRANCH": 0}, "model", {"cuda": [(("model", "branches", "light"), True, False)]}, {"cuda": MODEL})
ARMS["geom_branch_1"] = _arm({"HIFIHR_GEOM_BRANCH": 1}, "model", {"cuda": [(("model", "branches", "geom"), False, True)]}, {"cuda": MODEL})
ARMS["mano_fused_0"] = _arm({"HIFIHR_MANO_FUSED": 0}, "model",
                            {"cuda": [(("model", "calls", "mano_full_fwd"), True, False), (("model", "calls", "mano_joints_fwd"), False, True)]}, {"cuda": MODEL})

# ---- csrc/render_common.h -------------------------------------------------------------------------------------------------------------------
_RENDER = [("render", ("hand", "mano", 1, 16, 1, "vc")), ("render", ("hand", "mano", 3, 17, 2, "shared")), ("render", ("hand", "mano", 1, 33, 1, "uv")),
           ("render", ("offscreen", "mano", 6, 20, 2, "vc"))]
ARMS["render_tile_16"] = _arm(
    {"HIFIHR_RENDER_TILE": 16}, "cabi",
    {"cpu": [(("launched", "render", _RENDER[1][1], "render_fwd2_kernel<2,16,"), False, True), (("launched", "render", _RENDER[1][1], "render_fwd3_kernel<"), True, False)],
     "cuda": [(("profiled", "render", _RENDER[1][1], "render_fwd2_kernel<2,16,"), False, True), (("profiled", "render", _RENDER[1][1], "render_fwd3_kernel<"), True, False)]},
    {"cpu": _RENDER, "cuda": _RENDER})

ALL_SWITCHES = {k for a in ARMS.values() for k in a["env"]}


def witness(arm, device):
    """[(query, default answer, arm's answer)].  An arm's answer of None (a "conv_log" query): the default's log no longer passes in the arm's
    process, which is not asked; the arm's own, different log for the same case is asserted by a dispatch case of the arm."""
    return list(arm["witness"].get(device, []))


def cases(arm, device):
    return list(arm["cases"].get(device, []))


def devices(arm):
    return ("cpu", "cuda") if arm["level"] == "cabi" else ("cuda",)
