// Weight blob layout (little endian), written by spef_amd/blob.py -- keep the two in sync.
//
//   [BlobHeader 128 B][OpDesc 128 B x n_ops][pad to 256][data section: 256-B aligned tensors]
//
// Ops (reference module -> op):
//   OP_STEM  ConvBnAct 3->32 s2 (mobilenet_v2.py:252-254)   w0 fp32 [27][32] (k=ky*9+kx*3+ci), b0 fp32 [32]
//   OP_IRB   InvertedResidual (pytorch_layers.py:65-98)       w0/b0 expand 1x1: act [Np][Kp], fp32 [Np] (absent if t==1)
//                                                             w1/b1 depthwise: fp32 [9][hidden], fp32 [hidden]
//                                                             w2/b2 project 1x1: act [Np][Kp], fp32 [Np]
//   OP_LAST  ConvBnAct 320->1280 1x1 (mobilenet_v2.py:264)    w0 act [Np][Kp], b0 fp32 [Np]
//   OP_FC    URSONetHead ori|pos Linear (ursonet.py:17-25)    w0 fp32 [Np][1280] rows = ori then pos, b0 fp32 [Np]
//   OP_FCKP  KeypointRegressionHead (keypoints.py:18-21)      w0 fp32 [Np][F] columns in NHWC flatten order
//
// int8 blob (dtype 3; semantics oracle/int8_ref.py, params spef_amd/quant.py). RQ(n) = requant table over
// Np channels: int64 M[Np], int64 B[Np], int32 S[Np] back to back.
//   OP_QSTEM w0 int8 [32][28] (k=ky*9+kx*3+ci, k=27 zero), b0 RQ(32), w1 int8 LUT[256] (u8 pixel -> input
//            quant), x0 fp32 [1] input scale (f32 NCHW path)
//   OP_QIRB  w0/b0 expand int8 [Np][Kp64] + RQ (absent if t==1); w1/b1 dw int8 [9][hidden] + RQ;
//            w2/b2 project int8 [Np][Kp64] + RQ; x0 int32 [Np] project accumulator init (128 * sum_k q_w);
//            x1 int64 [3] residual-join rescale (R, RB, RS) when flags & 1; flags & 2: unsigned block input;
//            flags & 4: every x2 requant shift is exactly 32;
//            x2 fused-kernel tables (expand ops): RQ16 expand [H32] | RQ16 depthwise [H32] | RQ16 project [Np] |
//            depthwise weights fp16 [9][H32] (H32 = hidden rounded up to 32; RQ16 = {int32 M, int32 S, int64 B})
//   OP_QLAST w0 int8 [Np][Kp64], b0 RQ
//   OP_QFC   w0 int8 [Np][1280] (ori rows then pos), b0 fp64 [Np] weight scales, w1 fp64 [Np] float bias,
//            x0 int32 [Np] 128 * sum_k q_w, x1 fp64 [1] last-conv activation scale
// qbits (bit_width.json of the reference's QMobileNetV2 / QURSONetHead, model.py:16-45; 0 means 8; 3..8 allowed):
//   OP_QSTEM [0] first_conv activation (unsigned), [1] image (signed, f32 NCHW input path; the u8 LUT has it built in)
//   OP_QIRB  [0] expand activation, [1] depthwise activation (unsigned), [2] shared_act (signed output quantizer)
//   OP_QLAST [0] last_conv activation (unsigned), [1] pooling (TruncTo8bit output: shift = [0] + ceil(log2 HW) - [1])
//   OP_QFC   [0] fully_connected bias width (signed)
// act = the activation storage type (fp16, bf16 or fp32 -- dtype 4, whose depthwise weights are fp32 as in bf16
// blobs and whose stem x0 is fp32 hi + zero lo); Kp = K rounded up to 32, Np = N rounded up to 16, padding 0.
// fp16x2 blob (dtype 5, k_x2_*.hip; fp32 activations): every 1x1 weight is [2][rows][Kp] fp16 (hi plane = fp16(w), lo
// plane = fp16(w - hi)), expand rows padded to H32 = hidden rounded up to 32; depthwise fp32 [9][H32], expand and
// depthwise biases fp32 [H32]; stem x0 = [2][3 ky][32 ch][32 k] fp16 hi / lo of the /255-folded weights, k = 4 kx + ci.
// fp16mx blob (dtype 6): the dtype-5 layout; OP_STEM x1 = [2][32 ch][32 k] fp16 hi / lo of the /255-folded weights in
// the fp16 front kernel's row-triple k order (front_mx_kernel). The schedule stores the stem map, the block outputs of
// blocks 1-3 and the hidden tensors of blocks 2-4 in fp16.
// BatchNorm (eps 1e-5) is folded: w' = w*g/sqrt(v+eps), b' = beta - mean*g/sqrt(v+eps).
#pragma once
#include <stdint.h>

namespace spef {

static const char kBlobMagic[8] = {'S', 'P', 'E', 'F', 'M', 'I', '3', '5'};
static const uint32_t kBlobVersion = 2;   // 2: fp16 stem operand (x0) in the front_vp_kernel row-triple k order
static const uint64_t kAbsent = ~0ull;

enum OpKind : uint32_t {
  OP_STEM = 1, OP_IRB = 2, OP_LAST = 3, OP_FC = 4, OP_FCKP = 5,
  OP_QSTEM = 11, OP_QIRB = 12, OP_QLAST = 13, OP_QFC = 14   // int8 blob (dtype 3)
};
enum HeadKind : uint32_t { HEAD_URSONET = 0, HEAD_KEYPOINTS = 1 };

#pragma pack(push, 1)
struct BlobHeader {
  char magic[8];
  uint32_t version, dtype, head, n_ops;
  uint32_t n_out0, n_out1, feat_c, kp_fh, kp_fw, pad0;
  uint64_t ops_off, data_off, data_bytes;
  uint8_t reserved[56];
};
struct OpDesc {
  uint32_t kind, cin, cout, hidden, stride, expand, flags, pad0;
  uint64_t w0, b0, w1, b1, w2, b2;
  uint64_t x0, x1, x2;   // extra tensors (int8 ops; kAbsent otherwise)
  uint8_t qbits[4];      // int8 ops: quantizer bit widths (0 = 8), see below
  uint8_t reserved[20];
};
#pragma pack(pop)
static_assert(sizeof(BlobHeader) == 128, "BlobHeader must be 128 bytes");
static_assert(sizeof(OpDesc) == 128, "OpDesc must be 128 bytes");

}  // namespace spef
