// Blob validation and loading (include/spef.h): op_extents / parse_blob are pure host code; staging copies a parsed
// blob into fresh device storage and committing hands it to a context. tools/sanitize_blob.py compiles this file alone
// under the sanitizers.
#include <string.h>

#include <algorithm>

#include "spef_ctx.hpp"

// Minimum byte extent of each tensor an op references (w0, b0, w1, b1, w2, b2, x0, x1, x2), from the op
// geometry and the blob layout in spef_blob.hpp; 0 where the op has no such tensor.
static void op_extents(const OpDesc& op, uint32_t dtype, uint64_t ext[9]) {
  auto r16 = [](uint64_t n) { return (n + 15) & ~15ull; };
  auto r32 = [](uint64_t n) { return (n + 31) & ~31ull; };
  auto r64 = [](uint64_t n) { return (n + 63) & ~63ull; };
  const uint64_t a = dtype == DT_F32 ? 4 : 2;             // fp16 / bf16 | fp32 weight storage
  const uint64_t rq = 20;                                 // int64 M + int64 B + int32 S per channel
  for (int i = 0; i < 9; ++i) ext[i] = 0;
  const uint64_t ci = op.cin, co = op.cout, h = op.hidden;
  if (dtype == DT_X2 || dtype == DT_MX) {   // fp16x2 / fp16mx: 1x1 weights as [2][rows][Kp] fp16 planes (hi, lo);
                                            // depthwise / biases padded to 32
    switch (op.kind) {
      case OP_STEM:
        ext[0] = 27 * co * 4; ext[1] = co * 4; ext[6] = 2 * 3 * co * 32 * 2;
        if (dtype == DT_MX) ext[7] = 2 * co * 32 * 2;   // front_mx_kernel's operand (row-triple k order)
        break;
      case OP_IRB:
        if (op.expand != 1) { ext[0] = 2 * r32(h) * r32(ci) * 2; ext[1] = r32(h) * 4; }
        ext[2] = 9 * r32(h) * 4; ext[3] = r32(h) * 4;
        ext[4] = 2 * r16(co) * r32(h) * 2; ext[5] = r16(co) * 4;
        break;
      case OP_LAST: ext[0] = 2 * r16(co) * r32(ci) * 2; ext[1] = r16(co) * 4; break;
      case OP_FC: case OP_FCKP: ext[0] = r16(co) * ci * 4; ext[1] = r16(co) * 4; break;
      default: break;
    }
    return;
  }
  switch (op.kind) {
    case OP_STEM: ext[0] = 27 * co * 4; ext[1] = co * 4; ext[6] = 2 * co * 32 * a; break;
    case OP_IRB:
      if (op.expand != 1) { ext[0] = r16(h) * r32(ci) * a; ext[1] = r16(h) * 4; }
      ext[2] = 9 * h * (dtype == DT_F16 ? 2 : 4); ext[3] = h * 4;
      ext[4] = r16(co) * r32(h) * a; ext[5] = r16(co) * 4;
      break;
    case OP_LAST: ext[0] = r16(co) * r32(ci) * a; ext[1] = r16(co) * 4; break;
    case OP_FC: case OP_FCKP: ext[0] = r16(co) * ci * 4; ext[1] = r16(co) * 4; break;
    case OP_QSTEM: ext[0] = 32 * 28; ext[1] = 32 * rq; ext[2] = 256; ext[6] = 4; break;
    case OP_QIRB: {
      if (op.expand != 1) { ext[0] = r16(h) * r64(ci); ext[1] = r16(h) * rq; }
      ext[2] = 9 * h; ext[3] = r16(h) * rq;
      ext[4] = r16(co) * r64(h); ext[5] = r16(co) * rq;
      ext[6] = r16(co) * 4;
      if (op.flags & 1u) ext[7] = 24;
      if (op.x2 != kAbsent) ext[8] = 16 * r32(h) * 2 + 16 * r16(co) + 2 * 9 * r32(h);
      break;
    }
    case OP_QLAST: ext[0] = r16(co) * r64(ci); ext[1] = r16(co) * rq; break;
    case OP_QFC: ext[0] = r16(co) * ci; ext[1] = r16(co) * 8; ext[2] = r16(co) * 8; ext[6] = r16(co) * 4; ext[7] = 8; break;
    default: break;
  }
}

// Parse and validate a blob's header + op table (host bytes: at least the first `meta_bytes` of the blob; `bytes`
// is the whole blob's size). Pure host code -- writes nothing but *h / *ops, and only on success.
static int parse_blob(const uint8_t* head_bytes, size_t meta_bytes, size_t bytes, BlobHeader* h_out,
                      std::vector<OpDesc>* ops_out) {
  if (meta_bytes < sizeof(BlobHeader) || bytes < sizeof(BlobHeader)) return fail(SPEF_ERR_BLOB, "blob too small");
  BlobHeader h;
  memcpy(&h, head_bytes, sizeof(h));
  if (memcmp(h.magic, kBlobMagic, 8) != 0) return fail(SPEF_ERR_BLOB, "bad blob magic");
  if (h.version != kBlobVersion) return fail(SPEF_ERR_BLOB, "unsupported blob version");
  if (h.dtype != DT_F16 && h.dtype != DT_BF16 && h.dtype != DT_I8 && h.dtype != DT_F32 && h.dtype != DT_X2 &&
      h.dtype != DT_MX)
    return fail(SPEF_ERR_BLOB, "unsupported blob dtype");
  if (h.n_ops == 0 || h.n_ops > 4096) return fail(SPEF_ERR_BLOB, "bad op count");
  // every term bounded on its own before any sum (a crafted ops_off near 2^64 must not wrap ops_end)
  if (h.ops_off < sizeof(BlobHeader) || h.ops_off > bytes || (uint64_t)h.n_ops * sizeof(OpDesc) > bytes - h.ops_off)
    return fail(SPEF_ERR_BLOB, "blob truncated");
  const uint64_t ops_end = h.ops_off + (uint64_t)h.n_ops * sizeof(OpDesc);
  if (ops_end > h.data_off || h.data_off > bytes ||
      h.data_bytes > bytes - h.data_off || ops_end > meta_bytes)
    return fail(SPEF_ERR_BLOB, "blob truncated");
  if (h.feat_c != 1280) return fail(SPEF_ERR_BLOB, "feature width must be 1280 (mobilenet_v2.py:232)");
  std::vector<OpDesc> ops(h.n_ops);
  memcpy(ops.data(), head_bytes + h.ops_off, h.n_ops * sizeof(OpDesc));
  int n_head = 0;
  for (const OpDesc& op : ops) {
    uint64_t ext[9];
    op_extents(op, h.dtype, ext);
    const uint64_t offs[9] = {op.w0, op.b0, op.w1, op.b1, op.w2, op.b2, op.x0, op.x1, op.x2};
    for (int i = 0; i < 9; ++i) {
      if (offs[i] == kAbsent) {
        if (ext[i] && !(op.kind == OP_QIRB && i == 8)) return fail(SPEF_ERR_BLOB, "op lacks a required tensor");
        continue;
      }
      if ((offs[i] & 15) || offs[i] >= h.data_bytes || ext[i] > h.data_bytes - offs[i])
        return fail(SPEF_ERR_BLOB, "tensor extent out of range / misaligned (op kind " + std::to_string(op.kind) + ")");
    }
    if ((op.kind == OP_IRB || op.kind == OP_QIRB) &&
        (op.cin % 8 || op.cout % 8 || op.hidden % 8 || (op.stride != 1 && op.stride != 2)))
      return fail(SPEF_ERR_BLOB, "unsupported inverted-residual geometry");
    const bool qop = op.kind >= OP_QSTEM && op.kind <= OP_QFC;
    if (qop != (h.dtype == DT_I8)) return fail(SPEF_ERR_BLOB, "op kind does not match the blob dtype");
    if (op.kind == OP_QSTEM && op.cout != 32) return fail(SPEF_ERR_BLOB, "int8 stem needs 32 outputs");
    for (int k = 0; k < 4; ++k)
      if (op.qbits[k] == 1 || op.qbits[k] == 2 || op.qbits[k] > 8 || (op.qbits[k] && !qop))
        return fail(SPEF_ERR_BLOB, "quantizer bit widths must be 3..8 (int8 ops only; quant.check_bit_width)");
    if (op.kind == OP_FC || op.kind == OP_QFC) {
      ++n_head;
      if (h.head != HEAD_URSONET || op.cin != h.feat_c || op.cout != h.n_out0 + h.n_out1)
        return fail(SPEF_ERR_BLOB, "URSONet head widths do not match the header");
    }
    if (op.kind == OP_FCKP) {
      ++n_head;
      if (h.head != HEAD_KEYPOINTS || op.cout != h.n_out0 || op.cin != (uint64_t)h.kp_fh * h.kp_fw * h.feat_c)
        return fail(SPEF_ERR_BLOB, "keypoint head widths do not match the header");
    }
  }
  if (n_head != 1) return fail(SPEF_ERR_BLOB, "blob must hold exactly one head op");
  *h_out = h;
  *ops_out = std::move(ops);
  return SPEF_OK;
}

// Stage the blob at `blob` (host or device memory) into `st`.
int stage_blob(spef_ctx* c, const void* blob, size_t bytes, bool on_device, Staged* st) {
  if (!c || !blob) return fail(SPEF_ERR_ARG, "null argument");
  Dev d(c->device);
  std::vector<uint8_t> head;
  const uint8_t* hb;
  size_t meta;
  if (on_device) {   // header + op table live in the first bytes; fetch them to the host
    if (bytes < sizeof(BlobHeader)) return fail(SPEF_ERR_BLOB, "blob too small");
    BlobHeader h0;
    HIP_TRY(hipMemcpy(&h0, blob, sizeof(h0), hipMemcpyDeviceToHost));
    meta = std::max<size_t>(sizeof(h0), std::min<size_t>(bytes, (size_t)h0.data_off));
    head.resize(meta);
    HIP_TRY(hipMemcpy(head.data(), blob, meta, hipMemcpyDeviceToHost));
    hb = head.data();
  } else {
    hb = (const uint8_t*)blob;
    meta = bytes;
  }
  int rc = parse_blob(hb, meta, bytes, &st->h, &st->ops);
  if (rc) return rc;
  const BlobHeader& h = st->h;
  const std::vector<OpDesc>& ops = st->ops;
  HIP_TRY(hipMalloc(&st->dd, std::max<uint64_t>(h.data_bytes, 256)));
  uint8_t* dd = st->dd;
  const uint8_t* src = (const uint8_t*)blob + h.data_off;
  HIP_TRY(hipMemcpy(dd, src, h.data_bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  if (h.dtype == DT_I8) {   // small host-side constants of the int8 schedule, fetched once
    st->q8_res.assign(ops.size(), {0, 0, 0});
    for (size_t i = 0; i < ops.size(); ++i) {
      const OpDesc& op = ops[i];
      if (op.kind == OP_QSTEM) HIP_TRY(hipMemcpy(&st->q8_s_img, dd + op.x0, sizeof(float), hipMemcpyDeviceToHost));
      if (op.kind == OP_QLAST) {
        st->q8_last_bits = qbits(op, 0);
        st->q8_pool_bits = qbits(op, 1);
      }
      if (op.kind == OP_QFC) st->q8_fc_bias_bits = qbits(op, 0);
      if (op.kind == OP_QIRB && (op.flags & 1u))
        HIP_TRY(hipMemcpy(st->q8_res[i].data(), dd + op.x1, 3 * sizeof(int64_t), hipMemcpyDeviceToHost));
      if (op.kind == OP_QFC) {
        const size_t np_ = (op.cout + 15) & ~15u;
        st->q8_sw.resize(np_);
        st->q8_bias.resize(np_);
        st->q8_wsum.resize(np_);
        HIP_TRY(hipMemcpy(st->q8_sw.data(), dd + op.b0, np_ * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(st->q8_bias.data(), dd + op.w1, np_ * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(st->q8_wsum.data(), dd + op.x0, np_ * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&st->q8_sl, dd + op.x1, sizeof(double), hipMemcpyDeviceToHost));
      }
    }
  }
  return SPEF_OK;
}

// Second half: the context takes the staged model (cannot fail).
void commit_staged(spef_ctx* c, Staged* st) {
  Dev d(c->device);
  free_workspace(c);
  if (c->d_data) hipFree(c->d_data);
  c->d_data = st->dd;
  st->dd = nullptr;
  c->data_bytes = st->h.data_bytes;
  c->hdr = st->h;
  c->ops = std::move(st->ops);
  c->q8_res = std::move(st->q8_res);
  c->q8_sw = std::move(st->q8_sw);
  c->q8_bias = std::move(st->q8_bias);
  c->q8_wsum = std::move(st->q8_wsum);
  c->q8_sl = st->q8_sl;
  c->q8_s_img = st->q8_s_img;
  c->q8_last_bits = st->q8_last_bits;
  c->q8_pool_bits = st->q8_pool_bits;
  c->q8_fc_bias_bits = st->q8_fc_bias_bits;
  c->q8_fc_hw = 0;
  c->loaded = true;
}

extern "C" {

static int load_common(spef_ctx* c, const void* blob, size_t bytes, bool on_device) {
  Staged st;
  const int rc = stage_blob(c, blob, bytes, on_device, &st);
  if (rc) return rc;
  commit_staged(c, &st);
  return SPEF_OK;
}

int spef_load_weights(spef_ctx* c, const void* blob, size_t bytes) { return load_common(c, blob, bytes, false); }

int spef_load_weights_device(spef_ctx* c, const void* blob, size_t bytes) { return load_common(c, blob, bytes, true); }

int spef_validate_blob(const void* blob, size_t bytes, int* dtype, int* head, int* n_out0, int* n_out1) {
  if (!blob) return fail(SPEF_ERR_ARG, "null blob");
  BlobHeader h;
  std::vector<OpDesc> ops;
  const int rc = parse_blob((const uint8_t*)blob, bytes, bytes, &h, &ops);
  if (rc) return rc;
  if (dtype) *dtype = (int)h.dtype;
  if (head) *head = (int)h.head;
  if (n_out0) *n_out0 = (int)h.n_out0;
  if (n_out1) *n_out1 = (int)h.n_out1;
  return SPEF_OK;
}

}  // extern "C"
