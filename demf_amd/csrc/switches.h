// The library's A/B switches: ONE table - environment name, default, meaning - and one read.  sw() parses the
// environment once per process ("unset" = the default, otherwise atoi); every launch function reads sw().field.
// demf_switch_at (include/demf_hip.h) enumerates the same table for Python, tests and tools.  DESIGN_LOG.md, section 5
// has the measurements behind the defaults.
#pragma once

namespace demf {

//        field               environment name            default  meaning
#define DEMF_SWITCHES(X) \
  X(f32_native,         "DEMF_F32_NATIVE",         0,     "initial compute mode: 1 = fp32 MFMA (mode 0) instead of three bf16 terms (mode 2)") \
  X(f16_terms,          "DEMF_F16_TERMS",          1,     "initial two-fp16-term setting of mode 2 (demf_set_f16_terms overrides)") \
  X(f16_terms_bwd,      "DEMF_F16_TERMS_BWD",      1,     "fused backward: 0 = three bf16 terms, 1 = two fp16 terms, 2 = also the pool form") \
  X(x3_mask,            "DEMF_X3_MASK",            7,     "mode 2 per kernel family: bit 0 forward, bit 1 dX, bit 2 weight gradient") \
  X(static_tiles,       "DEMF_STATIC_TILES",       0,     "1 = static tile schedule, no BN-finalize ticket in the GEMM") \
  X(acc_repl,           "DEMF_ACC_REPL",           1,     "replicated statistics accumulators") \
  X(acc_repl_fwd,       "DEMF_ACC_REPL_FWD",       0,     "replicated accumulators in the forward finalize") \
  X(acc_repl_red,       "DEMF_ACC_REPL_RED",       0,     "replicated accumulators in the dX reduce finalize") \
  X(gemm_grid,          "DEMF_GEMM_GRID",          512,   "block cap of the persistent shared-MLP GEMM") \
  X(persist_cus,        "DEMF_PERSIST_CUS",        240,   "blocks of the weight-resident / producer-consumer forwards") \
  X(persist_cus_bwd,    "DEMF_PERSIST_CUS_BWD",    240,   "blocks of the fused backwards; unset = DEMF_PERSIST_CUS (reported value is the effective one)") \
  X(fwd_pc,             "DEMF_FWD_PC",             1,     "producer/consumer forward (K = 128)") \
  X(fwd_pc_min_r,       "DEMF_FWD_PC_MIN_R",       16384, "fewest rows for the producer/consumer forward") \
  X(fwd_res,            "DEMF_FWD_RES",            1,     "weight-resident forward (K = 64, N = 64 / 128)") \
  X(fwd_tile,           "DEMF_FWD_TILE",           1,     "few-row tile forward") \
  X(fwd_tile_max_r,     "DEMF_FWD_TILE_MAX_R",     16384, "most rows for the tile forward") \
  X(dx_tile,            "DEMF_DX_TILE",            1,     "few-row tile dX") \
  X(dx_tile_max_r,      "DEMF_DX_TILE_MAX_R",      16384, "most rows for the tile dX") \
  X(dx_chunks,          "DEMF_DX_CHUNKS",          0,     "chunked dX reduce") \
  X(pool_halves,        "DEMF_POOL_HALVES",        0,     "1 = ns 64 pooling on two co-scheduled column halves") \
  X(pool_dyn,           "DEMF_POOL_DYN",           1,     "dynamic tile schedule in the pooling GEMM") \
  X(x3_wide_split,      "DEMF_X3_WIDE_SPLIT",      1,     "0 = wide three-term forwards on the fp32 MFMA instead of a column split") \
  X(split_target,       "DEMF_SPLIT_TARGET",       256,   "blocks the column split aims at") \
  X(no_fin,             "DEMF_NO_FIN",             0,     "1 = no in-kernel BN finalize") \
  X(bnred_ns1_dense,    "DEMF_BNRED_NS1_DENSE",    1,     "dense form of the BN-backward reduce at ns = 1") \
  X(bnred_pooled_dense, "DEMF_BNRED_POOLED_DENSE", 1,     "dense form of the BN-backward reduce on pooled rows") \
  X(bnred_rpb,          "DEMF_BNRED_RPB",          8,     "rows per thread of the replicated dense reduce") \
  X(bnred_grid,         "DEMF_BNRED_GRID",         -1,    "block cap of the dense reduce; -1 = 1024 replicated, 256 otherwise") \
  X(bnred_rev,          "DEMF_BNRED_REV",          1,     "dense reduce visits its rows last to first") \
  X(bnred_sparse_rpt,   "DEMF_BNRED_SPARSE_RPT",   8,     "rows per thread of the sparse reduce") \
  X(bnred_sparse_grid,  "DEMF_BNRED_SPARSE_GRID",  1024,  "block cap of the sparse reduce") \
  X(dw_small_r,         "DEMF_DW_SMALL_R",         65536, "weight-gradient launches of at most this many rows use 64 x 64 sub-blocks") \
  X(dw_tile,            "DEMF_DW_TILE",            0,     "weight-gradient sub-block: 12 = 64 x 128, 21 = 128 x 64, 22, 11") \
  X(dw_f32,             "DEMF_DW_F32",             0,     "bf16 mode: weight gradient on fp32 operands") \
  X(dw_grid,            "DEMF_DW_GRID",            512,   "blocks of the grouped weight-gradient launch") \
  X(dw_dyn,             "DEMF_DW_DYN",             0,     "dynamic schedule of the weight-gradient launch") \
  X(dw_dbg,             "DEMF_DW_DBG",             0,     "weight gradient: phase-skip timing experiments") \
  X(dw_trace,           "DEMF_DW_TRACE",           0,     "print the step's weight-gradient products (tools/dw_micro.py)") \
  X(bwd_dbg,            "DEMF_BWD_DBG",            0,     "fused backward: phase-skip timing experiments") \
  X(pb_dbg,             "DEMF_PB_DBG",             0,     "pool backward: phase-skip timing experiments") \
  X(gemm_small_tiles,   "DEMF_GEMM_SMALL_TILES",   1024,  "demf_gemm_f32 launches of at most this many 64 x 64 tiles use the 32 x 32 kernel") \
  X(gemm_tn3,           "DEMF_GEMM_TN3",           1,     "0 = no three-term TN GEMM") \
  X(gemm_tn_split,      "DEMF_GEMM_TN_SPLIT",      0,     "forced K split of the TN GEMM") \
  X(tn_dbg,             "DEMF_TN_DBG",             0,     "TN GEMM: phase-skip timing experiments") \
  X(ln_bwd_blocks,      "DEMF_LN_BWD_BLOCKS",      256,   "blocks of the LayerNorm backward (at least 1)") \
  X(rg_dbg,             "DEMF_RG_DBG",             0,     "row GEMM chain: phase-skip timing experiments") \
  X(rg_ln128,           "DEMF_RG_LN128",           0,     "row GEMM chain: the 128-row LayerNorm form") \
  X(rg_waves8,          "DEMF_RG_WAVES8",          0,     "row GEMM chain: the 8-wave forms") \
  X(rg_add4,            "DEMF_RG_ADD4",            0,     "row GEMM chain: the adding form on 4 waves") \
  X(rg_one,             "DEMF_RG_ONE",             0,     "row GEMM chain: non-zero = one workgroup per CU") \
  X(conv_stream64,      "DEMF_CONV_STREAM64",      1,     "streaming 1x1 convolution at K = 64") \
  X(conv_streamk,       "DEMF_CONV_STREAMK",       3,     "streaming 1x1 convolution: bit 0 K = 128, bit 1 K = 256") \
  X(conv_stream_min,    "DEMF_CONV_STREAM_MIN",    16384, "fewest rows for the streaming convolution") \
  X(conv_wg3,           "DEMF_CONV_WG3",           0,     "three-plane convolutions: three workgroups per CU") \
  X(msda_head_wgs,      "DEMF_MSDA_HEAD_WGS",      256,   "workgroups the (scene, head)-major attention aims at") \
  X(msda_raw_lanes,     "DEMF_MSDA_RAW_LANES",     0,     "non-zero = 8 lanes per query in the raw form") \
  X(msda_xcd,           "DEMF_MSDA_XCD",           0,     "XCD-aware block order") \
  X(msda_nt,            "DEMF_MSDA_NT",            1,     "non-temporal loads of the raw offsets / logits") \
  X(gf_fwd_blocks,      "DEMF_GF_FWD_BLOCKS",      1024,  "block cap of the group-first forward") \
  X(gf_bwd_blocks,      "DEMF_GF_BWD_BLOCKS",      0,     "block cap of the group-first backward (0 = its own choice)") \
  X(gf_fin,             "DEMF_GF_FIN",             1,     "0 = group-first forward without the in-kernel finalize") \
  X(gf_recompute,       "DEMF_GF_RECOMPUTE",       1,     "0 = group-first backward reads stored activations") \
  X(gf_wacc,            "DEMF_GF_WACC",            1,     "0 = group-first backward without the in-kernel weight gradient") \
  X(colsum_rows,        "DEMF_COLSUM_ROWS",        64,    "fewest rows per block of the column sum") \
  X(invert_split,       "DEMF_INVERT_SPLIT",       1,     "invert_index as five launches when the lists leave LDS; 2 = from 32 768 entries, 0 = never") \
  X(three_nn_split,     "DEMF_THREE_NN_SPLIT",     1,     "split form of three_nn") \
  X(fps_check_split,    "DEMF_FPS_CHECK_SPLIT",    1,     "two-kernel form of the FPS order check") \
  X(fps_prune,          "DEMF_FPS_PRUNE",          1,     "box-pruned FPS on large clouds") \
  X(fps_pair,           "DEMF_FPS_PAIR",           -1,    "per-pair cached maxima: -1 = above 16 slots per lane, 0 / 1 force") \
  X(fps_pair_waves,     "DEMF_FPS_PAIR_WAVES",     16,    "waves of the pair kernel (8 or 16)") \
  X(fps_waves,          "DEMF_FPS_WAVES",          16,    "waves of the pruned kernel (8 or 16)")

struct Switches {
#define DEMF_SW_FIELD(field, name, dflt, meaning) int field;
  DEMF_SWITCHES(DEMF_SW_FIELD)
#undef DEMF_SW_FIELD
};

const Switches& sw();   // csrc/switches.hip: filled from the environment at the first call, once per process

}  // namespace demf
