// Internal kernel-tuning options of spef_set_option (not part of the public ABI in include/spef.h).
// Used by the sweep tools (tools/explore.py, tools/ab.py) to time alternative schedules on the GPU box.
//   SPEF_OPT_FUSE_MIN_HW: fuse only blocks whose input has at least this many pixels per image (the rest run as
//                         GEMM + depthwise + GEMM).
//   SPEF_OPT_PW_GEMM    : LDS-tiled MFMA GEMM (1, default) or register-direct kernel (0) for unfused 1x1 convs.
//   SPEF_OPT_IRB_VARIANT: fused-block tile variant (0 = tuned default).
//   SPEF_OPT_TEST_FAIL_BCAST: failure injection for spef_bcast_weights tests: 1 = this rank fails its local check
//                         before the data broadcast, 2 = fails staging after it, 3 = the header wait never completes
//                         (exercises the timeout -> ncclCommAbort path without a hung peer). 0 = off.
//   SPEF_OPT_MX_KERNELS : fp16mx blocks 2-7 on the dedicated kernels of k_mx.hip (1, default) or on the fp16x2 slab
//                         kernels with fp16 block I/O (0).
//   SPEF_OPT_TRIM       : kernels that drop work the result does not need, bit-identical to the ones they replace (an
//                         A/B switch, one bit per kernel). Bit 0: the fp16x2 / fp16mx last conv on the 128-pixel x
//                         320-channel staged tile (k_x2_pw.hip) instead of 64 x 256. Bit 1: the fp16mx blocks 2-4
//                         (k_mx.hip mx_irb_kernel) with the lean tile set-up -- scalar image bases, 32-bit per-lane
//                         offsets, incremental tile pixels, no bounds checks in interior workgroups -- instead of 64-bit
//                         per-pixel addresses (a map too large for the offsets runs the earlier form whatever the bit,
//                         under the profile key mx_irb_kernel_wide). Default 3 (all bits); a cleared bit runs the
//                         earlier kernel from the same build.
//   SPEF_OPT_X2_STAGE   : how the persistent role-split rows of the fp16x2 / fp16mx schedules (x2_plan.hpp kind 3:
//                         blocks 8-10 and 14) stage a chunk's weights. 1 (default): x2_irw_st_kernel -- every stage piece
//                         by LDS-DMA into static, separately named double buffers, kept in flight across the chunk
//                         barrier. 0: x2_irw_kernel -- register staging (blocks 8-10) / LDS-DMA into one dynamic array,
//                         drained every chunk (block 14). Bit-identical outputs, same plan and profile keys.
#pragma once

enum spef_tuning_option {
  SPEF_OPT_FUSE_MIN_HW = 2,
  SPEF_OPT_PW_GEMM = 3,
  SPEF_OPT_IRB_VARIANT = 4,
  SPEF_OPT_TEST_FAIL_BCAST = 5,
  SPEF_OPT_MX_KERNELS = 8,
  SPEF_OPT_TRIM = 9,
  SPEF_OPT_X2_STAGE = 10
};
