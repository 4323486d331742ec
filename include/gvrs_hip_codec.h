/*
 * gvrs_hip_codec.h -- C ABI of the MI355X-native GVRS tile codec (libgvrs_hip.so).
 *
 * This is the drop-in boundary for the Gridfour compression plug-in interface.
 * Reference paths are relative to core/src/main/java/org/gridfour/ of
 * gwlucastrig/gridfour.  The entry points are what a JNI binding of
 *     compress/ICompressionEncoder.java:61-91   (encode / encodeFloats)
 *     compress/ICompressionDecoder.java:62-105  (decode / decodeFloats)
 * would bind for the codec registered as "GvrsHuffman"
 * (compress/CodecHuffman.java:70-153, registered the way
 * gvrs/GvrsFileSpecification.java:1576-1631 addCompressionCodec does).
 * INTEGRATION.md shows the Java adapter + JNI stub a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types.
 *   - "host" entry points take host pointers and do their own H2D/D2H copies.
 *   - "dev" entry points take device pointers plus a HIP stream (hipStream_t
 *     passed as void*); they only enqueue work, never synchronise, never
 *     allocate (gf_context_reserve first) -> safe for hipGraph capture.
 *   - tiles are row-major int32[nRows*nCols], batches are contiguous tiles.
 *   - every function returns a gf_status; per-tile outcomes of batch calls are
 *     reported in a status array (int32 per tile).
 *   - bit-exactness contract: for every tile, the bytes produced equal the
 *     bytes CodecHuffman.encode returns for the same (codecIndex, nRows, nCols,
 *     values), and decode inverts CodecHuffman.decode exactly.
 *   - there is NO CPU fallback: without a usable HIP device every compute
 *     entry point returns GF_ERR_NO_DEVICE.
 */
#ifndef GVRS_HIP_CODEC_H
#define GVRS_HIP_CODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gf_status {
    GF_OK = 0,
    GF_DECLINED = 1,          /* encoder result is Java `null` (all cells null): CodecHuffman.java:80-82 */
    GF_OVERFLOW = 2,          /* packing longer than the slot/capacity handed in; length is still reported */
    GF_ERR_FORMAT = -1,       /* decoder: Java would throw IOException (CodecHuffman.java:155-169)        */
    GF_ERR_BOUNDS = -2,       /* Java would throw ArrayIndexOutOfBounds (short packing, nCols < 2, ...)   */
    GF_ERR_CAPACITY = -3,     /* host output buffer too small                                             */
    GF_ERR_ARG = -4,
    GF_ERR_NO_DEVICE = -5,    /* no HIP device / HIP runtime error at context creation                    */
    GF_ERR_HIP = -6,          /* a HIP call failed; gf_last_error() has the text                          */
    GF_ERR_UNSUPPORTED = -7
} gf_status;

/* INT4_NULL_CODE, util/GridfourConstants.java:61 */
#define GF_INT4_NULL ((int32_t)0x80000000)

/* predictor codes, compress/PredictorModelType.java:46-63 */
#define GF_PM_DIFFERENCING 1
#define GF_PM_LINEAR 2
#define GF_PM_TRIANGLE 3
#define GF_PM_DIFFERENCING_NULLS 4
/* predictor_mask bit for model m is 1 << (m-1); GF_PM_ALL = reference behaviour */
#define GF_PM_ALL 0xF

typedef struct gf_context gf_context;

/* ---- library / device ---- */
const char *gf_version(void);
const char *gf_status_string(int status);
/* text of the last HIP error seen by the calling thread ("" if none) */
const char *gf_last_error(void);
/* number of visible HIP devices (0 when there is none; never fails) */
int gf_device_count(void);

/* One context per (process, device): owns a stream and the scratch workspace.
 * A context may be called from several threads at once, as the reference calls
 * one codec instance from its tile cache and its decompression assistant
 * (gvrs/RasterTileCache.java:418-421, TileDecompressionAssistant.java:68-73):
 * every entry point that takes a context holds the context's lock for its
 * duration, so such calls run one after the other.  The *_dev entry points
 * return while their kernels are still queued on the context's stream; a
 * caller that hands them another stream orders that stream itself.  Different
 * contexts are independent (this is how tile batches shard over the GPUs of a
 * node).                                                                      */
gf_status gf_context_create(int device, gf_context **ctx);
void gf_context_destroy(gf_context *ctx);
/* pre-allocates the workspace (decode: M32 spill per resident workgroup, per-tile records of the tree / code-length
 * pre-pass kernels; encode: per-tile selection records between the two encoder kernels) for batches up to n_tiles tiles
 * of n_rows x n_cols; without it the first larger _dev call grows it */
gf_status gf_context_reserve(gf_context *ctx, int n_rows, int n_cols, size_t n_tiles);
/* the context's own stream (hipStream_t) */
void *gf_context_stream(gf_context *ctx);
gf_status gf_context_synchronize(gf_context *ctx);

/* slot stride (bytes, multiple of 16) the batch encoders use by default:
 * room for any packing the caller would keep (RasterTile keeps a packing only
 * when shorter than 4*cells, gvrs/TileElementInt.java:198-204).              */
size_t gf_huffman_default_stride(int n_rows, int n_cols);
/* absolute worst-case packing size of CodecHuffman for a tile */
size_t gf_huffman_max_packing(int n_rows, int n_cols);

/* ---- single tile, host memory: replaces ICompressionEncoder.encode /
 *      ICompressionDecoder.decode as implemented by CodecHuffman ----------- */
/* returns GF_OK, GF_DECLINED (Java null), GF_ERR_CAPACITY (out_len = needed) */
gf_status gf_huffman_encode_i32(gf_context *ctx, int codec_index, int n_rows, int n_cols,
                                const int32_t *values, uint8_t *out, size_t out_cap,
                                size_t *out_len);
/* returns GF_OK or GF_ERR_FORMAT / GF_ERR_BOUNDS (Java IOException / AIOOBE) */
gf_status gf_huffman_decode_i32(gf_context *ctx, int n_rows, int n_cols,
                                const uint8_t *packing, size_t packing_len, int32_t *values);

/* ---- batches, host memory --------------------------------------------- */
/* Encodes n_tiles tiles.  Packings are concatenated in tile order into blob;
 * offsets[n_tiles+1] receives their byte offsets (offsets[t+1]-offsets[t] = length,
 * 0 for a declined tile).  predictors[n_tiles] (optional) receives the predictor
 * code chosen per tile, status[n_tiles] (optional) the per-tile gf_status.
 * Returns GF_ERR_CAPACITY (offsets still filled) when blob_cap is too small.  */
gf_status gf_huffman_encode_batch_i32(gf_context *ctx, int codec_index, int n_rows, int n_cols,
                                      size_t n_tiles, const int32_t *values, uint8_t *blob,
                                      size_t blob_cap, uint64_t *offsets, uint8_t *predictors,
                                      int32_t *status);
gf_status gf_huffman_decode_batch_i32(gf_context *ctx, int n_rows, int n_cols, size_t n_tiles,
                                      const uint8_t *blob, const uint64_t *offsets,
                                      int32_t *values, int32_t *status);

/* ---- batches, device-resident (the measured hot path) ------------------ */
/* d_values  : n_tiles * n_rows*n_cols int32
 * d_out     : n_tiles slots of slot_stride bytes (16-byte aligned base, stride % 16 == 0);
 *             tile t's packing starts at t*slot_stride
 * d_lengths : packing length per tile (bytes; 0 = declined)
 * d_predictors (optional, may be NULL), d_status: per tile
 * predictor_mask: GF_PM_ALL for reference behaviour; a subset restricts the
 *             models tried (test hook, mirrors the oracle)
 * A tile reported GF_OVERFLOW or GF_DECLINED leaves its slot untouched: no byte
 * of the slot is written (d_lengths[t] is the full length for GF_OVERFLOW, 0 for
 * GF_DECLINED).  A tile reported GF_OK writes inside its own slot only.  This
 * holds for every _dev encoder that writes into slots (gf_huffman_*, gf_canon_*,
 * gf_lsop12_*; gf_m32_* per sub-slot, see there).                             */
gf_status gf_huffman_encode_batch_i32_dev(gf_context *ctx, void *stream, int codec_index,
                                          int n_rows, int n_cols, size_t n_tiles,
                                          const int32_t *d_values, uint8_t *d_out,
                                          size_t slot_stride, uint32_t *d_lengths,
                                          uint8_t *d_predictors, int32_t *d_status,
                                          int predictor_mask);
/* tile t's packing = d_blob[d_offsets[t] .. d_offsets[t]+d_lengths[t]).  When
 * d_offsets is NULL the packings sit in slots: offset = t*slot_stride.
 * d_blob must be 4-byte aligned; blob_bytes = readable size of d_blob.       */
gf_status gf_huffman_decode_batch_i32_dev(gf_context *ctx, void *stream, int n_rows, int n_cols,
                                          size_t n_tiles, const uint8_t *d_blob,
                                          size_t blob_bytes, const uint64_t *d_offsets,
                                          size_t slot_stride, const uint32_t *d_lengths,
                                          int32_t *d_values, int32_t *d_status);
/* Gathers slot-strided packings into one contiguous blob (exclusive scan of the
 * lengths + copy): d_offsets[n_tiles+1], d_blob capacity blob_cap bytes.      */
gf_status gf_compact_dev(gf_context *ctx, void *stream, size_t n_tiles, const uint8_t *d_slots,
                         size_t slot_stride, const uint32_t *d_lengths, uint64_t *d_offsets,
                         uint8_t *d_blob, size_t blob_cap);

/* gf_compact_dev cannot report a blob that is too small without synchronising: a packing that would end behind blob_cap
 * is skipped; d_offsets[n_tiles] > blob_cap tells the caller (after its own synchronisation) that this happened.
 * A tile with d_lengths[t] > slot_stride -- what a _dev encoder leaves behind for a tile it reported GF_OVERFLOW, whose
 * slot it did not write -- contributes no bytes: d_offsets[t+1] == d_offsets[t], as for a declined tile (length 0).
 * The caller tells the two apart by d_lengths[t] or the encoder's status array.                                          */

/* ---- page-locked host memory ---------------------------------------------------------------------------------------
 * The host-memory batch entry points cut a batch into chunks of about 64 MB of cells and pipeline them through three
 * slots (copy-in of chunk k+1, device work of chunk k and copy-out of chunk k-1 overlap; device and staging memory are
 * bounded by the chunk, not by the batch).  Pageable memory is staged through page-locked buffers by helper threads;
 * memory obtained here (a JNI binding hands it to Java as a direct ByteBuffer) moves over PCIe in place.               */
gf_status gf_host_alloc(size_t bytes, void **p);
gf_status gf_host_free(void *p);

/* ---- zlib (RFC 1950 / 1951) streams inflated on the GPU, one wave per stream -------------------------------------------
 * Replaces the java.util.zip.Inflater calls of the Deflate-carrying decoders (compress/CodecDeflate.java:141-147,
 * compress/CodecFloat.java:285-298, lsop/LsDecoder12.java:127-141).  Stream i is d_in[in_offsets[i] .. + in_lengths[i]);
 * at most out_caps[i] bytes go to d_out + out_offsets[i]; d_produced[i] = bytes written, d_status[i] = GF_OK or GF_ERR_FORMAT
 * -- the outcome of ONE Inflater.inflate(byte[]) call on the whole input: it stops without error when room or input run
 * out, reports invalid data where zlib does (DataFormatException) and verifies the Adler-32 when the stream ends inside
 * the room.  The four descriptor arrays are host arrays; d_in, d_out, d_produced, d_status are device memory.
 * Unlike the other _dev entry points this one ALLOCATES and BLOCKS: it uploads the descriptor arrays (a context-owned device
 * buffer that grows on demand: hipMalloc on first use and when n_streams grows; a pageable-memory copy that the host waits
 * for), so it is not capture-safe and is not covered by gf_context_reserve.  d_in must be 4-byte aligned and readable up to
 * the end of the aligned dword that holds the last byte of every stream: the kernel reads whole aligned dwords, i.e. up to
 * three bytes before a stream's first and after its last byte are touched (never used) -- leave 4 bytes of padding behind
 * the last stream of an allocation.                                                                                     */
gf_status gf_inflate_batch_dev(gf_context *ctx, void *stream, size_t n_streams, const uint8_t *d_in,
                               const uint64_t *in_offsets, const uint32_t *in_lengths, uint8_t *d_out,
                               const uint64_t *out_offsets, const uint32_t *out_caps, uint32_t *d_produced,
                               int32_t *d_status);

/* Deflate-carrying packings decoded entirely on the device (container walk, inflate, decode; scratch bounded by chunks):
 * CodecDeflate (layout as gf_huffman_decode_batch_i32_dev) and CodecFloat (d_offsets required).  The host-memory forms
 * gf_deflate_decode_batch_i32 / gf_float_decode_batch_f32 run the same kernels behind the pipelined staging.           */
gf_status gf_deflate_decode_batch_i32_dev(gf_context *ctx, void *stream, int n_rows, int n_cols, size_t n_tiles,
                                          const uint8_t *d_blob, size_t blob_bytes, const uint64_t *d_offsets,
                                          size_t slot_stride, const uint32_t *d_lengths, int32_t *d_values, int32_t *d_status);
gf_status gf_float_decode_batch_f32_dev(gf_context *ctx, void *stream, int n_rows, int n_cols, size_t n_tiles,
                                        const uint8_t *d_blob, size_t blob_bytes, const uint64_t *d_offsets,
                                        const uint32_t *d_lengths, float *d_values, int32_t *d_status);

/* ---- several GPUs from one process -----------------------------------------------------------------
 * What gvrs/CodecMaster.java:142-203 / gvrs/RecordManager.java:386-490 would call to use a whole node from one JVM.
 * A gf_multi owns one gf_context per listed device (a device may be listed more than once).  A batch of T tiles shards
 * as contiguous ranges, shard g = tiles [g T / G, (g+1) T / G) (gf_multi_partition); tiles are independent
 * (gvrs/RasterTile.java:237-241), so there is no exchange between devices and no collective.
 *   gf_*_batch_i32_multi      host memory: one host thread per context runs the pipelined host path on its range; the
 *                             packings are concatenated by an exclusive scan of the range totals.  Arguments, results and
 *                             bytes are those of the single-context call on the whole batch.
 *   gf_*_batch_i32_multi_dev  device memory: every array argument has gf_multi_count() entries, entry g lives on
 *                             gf_multi_device(g); the call enqueues each shard on its device's stream and returns;
 *                             gf_multi_synchronize waits for all devices.                                             */
typedef struct gf_multi gf_multi;
gf_status gf_multi_create(const int *devices, int n_devices, gf_multi **multi);
void gf_multi_destroy(gf_multi *multi);
int gf_multi_count(const gf_multi *multi);
gf_context *gf_multi_context(gf_multi *multi, int i);
int gf_multi_device(const gf_multi *multi, int i);
void gf_multi_partition(size_t n_tiles, int n_shards, int i, size_t *t0, size_t *t1);
gf_status gf_multi_synchronize(gf_multi *multi);
gf_status gf_huffman_encode_batch_i32_multi(gf_multi *multi, int codec_index, int n_rows, int n_cols, size_t n_tiles,
                                            const int32_t *values, uint8_t *blob, size_t blob_cap, uint64_t *offsets,
                                            uint8_t *predictors, int32_t *status);
gf_status gf_huffman_decode_batch_i32_multi(gf_multi *multi, int n_rows, int n_cols, size_t n_tiles, const uint8_t *blob,
                                            const uint64_t *offsets, int32_t *values, int32_t *status);
gf_status gf_canon_encode_batch_i32_multi(gf_multi *multi, int codec_index, int n_rows, int n_cols, size_t n_tiles,
                                          const int32_t *values, uint8_t *blob, size_t blob_cap, uint64_t *offsets,
                                          uint8_t *predictors, int32_t *status);
gf_status gf_canon_decode_batch_i32_multi(gf_multi *multi, int n_rows, int n_cols, size_t n_tiles, const uint8_t *blob,
                                          const uint64_t *offsets, int32_t *values, int32_t *status);
/* the same partition for the other codecs (CodecDeflate; LSOP12 -- BASELINE config 5(ii) sharded; CodecFloat -- config 5(i)):
 * arguments as the single-context entry points of the same name without _multi                                          */
gf_status gf_deflate_encode_batch_i32_multi(gf_multi *multi, int codec_index, int n_rows, int n_cols, size_t n_tiles,
                                            const int32_t *values, uint8_t *blob, size_t blob_cap, uint64_t *offsets,
                                            uint8_t *predictors, int32_t *status);
gf_status gf_deflate_decode_batch_i32_multi(gf_multi *multi, int n_rows, int n_cols, size_t n_tiles, const uint8_t *blob,
                                            const uint64_t *offsets, int32_t *values, int32_t *status);
gf_status gf_lsop12_encode_batch_i32_multi(gf_multi *multi, int codec_index, int n_rows, int n_cols, size_t n_tiles,
                                           const int32_t *values, int deflate_enabled, uint8_t *blob, size_t blob_cap,
                                           uint64_t *offsets, uint8_t *types, int32_t *status);
gf_status gf_lsop12_decode_batch_i32_multi(gf_multi *multi, int n_rows, int n_cols, size_t n_tiles, const uint8_t *blob,
                                           const uint64_t *offsets, int32_t *values, int32_t *status);
gf_status gf_float_encode_batch_f32_multi(gf_multi *multi, int codec_index, int n_rows, int n_cols, size_t n_tiles,
                                          const float *values, int zlib_level, uint8_t *blob, size_t blob_cap,
                                          uint64_t *offsets);
gf_status gf_float_decode_batch_f32_multi(gf_multi *multi, int n_rows, int n_cols, size_t n_tiles, const uint8_t *blob,
                                          const uint64_t *offsets, float *values, int32_t *status);
gf_status gf_canon_encode_batch_i32_multi_dev(gf_multi *multi, int codec_index, int n_rows, int n_cols,
                                              const size_t *n_tiles, const int32_t *const *d_values, uint8_t *const *d_out,
                                              size_t slot_stride, uint32_t *const *d_lengths, uint8_t *const *d_predictors,
                                              int32_t *const *d_status, int predictor_mask);
gf_status gf_canon_decode_batch_i32_multi_dev(gf_multi *multi, int n_rows, int n_cols, const size_t *n_tiles,
                                              const uint8_t *const *d_blob, const size_t *blob_bytes,
                                              const uint64_t *const *d_offsets, size_t slot_stride,
                                              const uint32_t *const *d_lengths, int32_t *const *d_values,
                                              int32_t *const *d_status);
gf_status gf_huffman_encode_batch_i32_multi_dev(gf_multi *multi, int codec_index, int n_rows, int n_cols,
                                                const size_t *n_tiles, const int32_t *const *d_values, uint8_t *const *d_out,
                                                size_t slot_stride, uint32_t *const *d_lengths, uint8_t *const *d_predictors,
                                                int32_t *const *d_status, int predictor_mask);
gf_status gf_huffman_decode_batch_i32_multi_dev(gf_multi *multi, int n_rows, int n_cols, const size_t *n_tiles,
                                                const uint8_t *const *d_blob, const size_t *blob_bytes,
                                                const uint64_t *const *d_offsets, size_t slot_stride,
                                                const uint32_t *const *d_lengths, int32_t *const *d_values,
                                                int32_t *const *d_status);

/* ---- CodecCanonHuffman (compress/canonicalHuffman/CodecCanonHuffman.java:70-195), the default integer
 * codec of current Gridfour (gvrs/GvrsFileSpecification.java:229): same predictors, integer residuals coded
 * with the 260-symbol canonical Huffman stage (CanonicalHuffman.java:177-283, 441-519), 6-byte header
 * codec_index, predictor, seed LE; uniform tiles pack to 6 bytes with predictor 0 (:95-110).
 * Same calling conventions, layouts and statuses as the gf_huffman_* entry points; additionally
 * GF_ERR_ARG where the Java encoder throws IllegalArgumentException (Triangle on a one-row tile, :183)
 * and GF_ERR_UNSUPPORTED for tiles of 2^20 cells or more.                                             */
size_t gf_canon_max_packing(int n_rows, int n_cols);
gf_status gf_canon_encode_i32(gf_context *ctx, int codec_index, int n_rows, int n_cols, const int32_t *values,
                              uint8_t *out, size_t out_cap, size_t *out_len);
gf_status gf_canon_decode_i32(gf_context *ctx, int n_rows, int n_cols, const uint8_t *packing, size_t packing_len,
                              int32_t *values);
gf_status gf_canon_encode_batch_i32(gf_context *ctx, int codec_index, int n_rows, int n_cols, size_t n_tiles,
                                    const int32_t *values, uint8_t *blob, size_t blob_cap, uint64_t *offsets,
                                    uint8_t *predictors, int32_t *status);
gf_status gf_canon_decode_batch_i32(gf_context *ctx, int n_rows, int n_cols, size_t n_tiles, const uint8_t *blob,
                                    const uint64_t *offsets, int32_t *values, int32_t *status);
gf_status gf_canon_encode_batch_i32_dev(gf_context *ctx, void *stream, int codec_index, int n_rows, int n_cols,
                                        size_t n_tiles, const int32_t *d_values, uint8_t *d_out, size_t slot_stride,
                                        uint32_t *d_lengths, uint8_t *d_predictors, int32_t *d_status,
                                        int predictor_mask);
gf_status gf_canon_decode_batch_i32_dev(gf_context *ctx, void *stream, int n_rows, int n_cols, size_t n_tiles,
                                        const uint8_t *d_blob, size_t blob_bytes, const uint64_t *d_offsets,
                                        size_t slot_stride, const uint32_t *d_lengths, int32_t *d_values,
                                        int32_t *d_status);

/* ---- CodecDeflate (compress/CodecDeflate.java:108-228): predictor -> CodecM32 on the GPU, Deflate (level 6) on the host's
 * zlib, 10-byte header codec_index, predictor, seed LE, nM32 LE.  The encoder deflates the M32 stream of every applicable
 * predictor and keeps the strictly shortest packing (:176-199).  The predictor + M32 stage is available on its own:
 *   gf_m32_encode_batch_i32_dev: per tile three candidate streams (sub-slots of sub_stride bytes, order Differencing, Linear,
 *     Triangle; a tile with nulls has the DifferencingWithNulls stream in sub-slot 0), d_lengths[3 n], d_models[3 n]
 *     (predictor code, 0 = no candidate), d_seeds[n].  A candidate stream is written only when length + 8 <= sub_stride:
 *     the packer stores whole 32-bit words, up to 8 bytes behind the stream's last byte.  gf_m32_default_stride and
 *     gf_m32_max_stream include that margin.  A candidate with length + 8 > sub_stride leaves its sub-slot untouched
 *     and makes the tile's status GF_OVERFLOW (every length is still exact; the tile's other candidates, where they
 *     fit, are written).
 *   gf_m32_decode_batch_i32_dev: "raw" containers = 10-byte CodecDeflate/CodecHuffman header followed by the M32 bytes
 *     themselves -> tiles (the stage after Inflater.inflate, CodecDeflate.java:141-147); layout as gf_huffman_decode_batch_i32_dev. */
size_t gf_m32_default_stride(int n_rows, int n_cols);
size_t gf_m32_max_stream(int n_rows, int n_cols);
gf_status gf_m32_encode_batch_i32_dev(gf_context *ctx, void *stream, int n_rows, int n_cols, size_t n_tiles,
                                      const int32_t *d_values, uint8_t *d_streams, size_t sub_stride, uint32_t *d_lengths,
                                      uint8_t *d_models, uint32_t *d_seeds, int32_t *d_status);
gf_status gf_m32_decode_batch_i32_dev(gf_context *ctx, void *stream, int n_rows, int n_cols, size_t n_tiles,
                                      const uint8_t *d_blob, size_t blob_bytes, const uint64_t *d_offsets, size_t slot_stride,
                                      const uint32_t *d_lengths, int32_t *d_values, int32_t *d_status);
gf_status gf_deflate_encode_batch_i32(gf_context *ctx, int codec_index, int n_rows, int n_cols, size_t n_tiles,
                                      const int32_t *values, uint8_t *blob, size_t blob_cap, uint64_t *offsets,
                                      uint8_t *predictors, int32_t *status);
gf_status gf_deflate_decode_batch_i32(gf_context *ctx, int n_rows, int n_cols, size_t n_tiles, const uint8_t *blob,
                                      const uint64_t *offsets, int32_t *values, int32_t *status);
gf_status gf_deflate_encode_i32(gf_context *ctx, int codec_index, int n_rows, int n_cols, const int32_t *values,
                                uint8_t *out, size_t out_cap, size_t *out_len);
gf_status gf_deflate_decode_i32(gf_context *ctx, int n_rows, int n_cols, const uint8_t *packing, size_t packing_len,
                                int32_t *values);

/* ---- LSOP12 (lsop/LsEncoder12.java:122-219, lsop/LsDecoder12.java:94-160, lsop/LsOptimalPredictor12.java:109-383,
 * lsop/LsHeader.java:131-265, util/jama/LUDecomposition.java:70-134, 253-284): the optimal 12-coefficient linear
 * predictor.  Tiles need at least 6 rows and 6 columns (else GF_DECLINED, Java null); a singular system is GF_DECLINED too.
 *   residuals: per tile res_stride ints (>= gf_lsop12_residual_count): [4R+2C-9 initialisers | (R-2)(C-4) interior]
 *   coefs:     per tile 16 words: seed, the 12 float32 coefficients as bit patterns, 3 spare
 * The encoder writes the current container: header (LsHeader.packHeader) + CanonicalHuffman of the two integer streams
 * in one bit store (compression type 2).  The Deflate alternative (type 1, LsEncoder12.java:180-216) is produced by the
 * host entry points with the host's zlib when deflate_enabled != 0 (the reference's default).  Decoding accepts every
 * container the reference's decoder does (LsDecoder12.java:107-150), with either header revision: type 2 and type 0
 * (legacy Huffman of the two M32 streams, what Sample14_LSOP.gvrs holds) and type 1 (two zlib streams, inflated on the
 * device: the second one starts where the first Inflater stopped reading) -- all of them entirely on the GPU, in the host
 * and the _dev forms alike.  The _dev decode allocates inflate scratch inside the context on first use (not capture-safe
 * until it has run once for the shape).                                                                             */
size_t gf_lsop12_residual_count(int n_rows, int n_cols);
size_t gf_lsop12_max_packing(int n_rows, int n_cols);
/* LsEncoder12's two switches, as bits of the `deflate_enabled` / `flags` argument of the encode entry points:
 *   GF_LSOP_DEFLATE         setDeflateEnabled (lsop/LsEncoder12.java:92-94, default on; 1, as the argument always meant)
 *   GF_LSOP_VALUE_CHECKSUM  setValueChecksumEnabled (:117-119, default off): LsHeader.computeChecksum (LsHeader.java:391-406), the
 *                           CRC-32C of the tile's values as little-endian bytes, computed on the device, goes behind the
 *                           header's last field and bit 7 of byte 1 is set (LsHeader.packHeader :245-262).  The decoders skip
 *                           it, as the reference's decoder only prints a mismatch (LsDecoder12.java:153-158).                */
#define GF_LSOP_DEFLATE 1
#define GF_LSOP_VALUE_CHECKSUM 2
/* ABI note: `deflate_enabled` was a boolean before the value checksum existed (any non-zero value meant Deflate); it is a bit mask of
 * the two switches above now -- 2 is "checksum, no Deflate", not "Deflate" -- and any other bit is refused with GF_ERR_ARG by every
 * encode entry point (the _dev_ex form accepts GF_LSOP_DEFLATE and ignores it: Deflate needs the host's zlib).               */
/* LsOptimalPredictor12.encode: tile -> coefficients + residual streams (d_status: GF_OK / GF_DECLINED per tile) */
gf_status gf_lsop12_predict_dev(gf_context *ctx, void *stream, int n_rows, int n_cols, size_t n_tiles,
                                const int32_t *d_values, int32_t *d_residuals, size_t res_stride, uint32_t *d_coefs,
                                int32_t *d_status);
/* LsDecoder12.unpackInitializers + unpackInterior: residual streams -> tile.  d_in_status (may be NULL): tiles whose
 * entry is not GF_OK are skipped and that value is passed through to d_status.  A tile's 16 words of d_coefs: seed,
 * the 12 float bit patterns, then words 13 .. 15, which a caller-built record must set to 0 (gf_lsop12_predict_dev
 * writes 0 there).  The d_residuals / d_coefs that gf_lsop12_decode_batch_i32_dev leaves behind are valid input.      */
gf_status gf_lsop12_reconstruct_dev(gf_context *ctx, void *stream, int n_rows, int n_cols, size_t n_tiles,
                                    const int32_t *d_residuals, size_t res_stride, const uint32_t *d_coefs,
                                    const int32_t *d_in_status, int32_t *d_values, int32_t *d_status);
/* device-resident batches; d_residuals / d_coefs / d_scratch_status (n_tiles ints) are caller-provided work buffers */
gf_status gf_lsop12_encode_batch_i32_dev(gf_context *ctx, void *stream, int codec_index, int n_rows, int n_cols,
                                         size_t n_tiles, const int32_t *d_values, uint8_t *d_out, size_t slot_stride,
                                         uint32_t *d_lengths, int32_t *d_status, int32_t *d_residuals, size_t res_stride,
                                         uint32_t *d_coefs, int32_t *d_scratch_status);
/* ... with flags (GF_LSOP_VALUE_CHECKSUM; the Deflate alternative is a host-side operation) */
gf_status gf_lsop12_encode_batch_i32_dev_ex(gf_context *ctx, void *stream, int codec_index, int n_rows, int n_cols,
                                            size_t n_tiles, const int32_t *d_values, int flags, uint8_t *d_out,
                                            size_t slot_stride, uint32_t *d_lengths, int32_t *d_status, int32_t *d_residuals,
                                            size_t res_stride, uint32_t *d_coefs, int32_t *d_scratch_status);
/* (the work buffers' contents behind a decode are the library's business: a tile's slot of d_residuals holds its initialisers and either
   its interior residuals as ints or -- tiles whose residuals are all bytes -- a byte plane in the order the reconstruction consumes it; words
   13 .. 15 of a tile's 16 words of d_coefs are the library's too) */
gf_status gf_lsop12_decode_batch_i32_dev(gf_context *ctx, void *stream, int n_rows, int n_cols, size_t n_tiles,
                                         const uint8_t *d_blob, size_t blob_bytes, const uint64_t *d_offsets,
                                         size_t slot_stride, const uint32_t *d_lengths, int32_t *d_values,
                                         int32_t *d_status, int32_t *d_residuals, size_t res_stride, uint32_t *d_coefs,
                                         int32_t *d_scratch_status);
/* host memory: replace LsEncoder12.encode / LsDecoder12.decode.  types[n_tiles] (optional): container type written */
gf_status gf_lsop12_encode_batch_i32(gf_context *ctx, int codec_index, int n_rows, int n_cols, size_t n_tiles,
                                     const int32_t *values, int deflate_enabled, uint8_t *blob, size_t blob_cap,
                                     uint64_t *offsets, uint8_t *types, int32_t *status);
gf_status gf_lsop12_decode_batch_i32(gf_context *ctx, int n_rows, int n_cols, size_t n_tiles, const uint8_t *blob,
                                     const uint64_t *offsets, int32_t *values, int32_t *status);
gf_status gf_lsop12_encode_i32(gf_context *ctx, int codec_index, int n_rows, int n_cols, const int32_t *values,
                               int deflate_enabled, uint8_t *out, size_t out_cap, size_t *out_len);
gf_status gf_lsop12_decode_i32(gf_context *ctx, int n_rows, int n_cols, const uint8_t *packing, size_t packing_len,
                               int32_t *values);

/* ---- LSOP08 (lsop/LsEncoder08.java:66-137, lsop/LsDecoder08.java:71-163, lsop/LsOptimalPredictor08.java:56-246,
 * lsop/LsHeader.java:137-265, util/jama/LUDecomposition.java:70-134, 253-284): the optimal 8-coefficient linear predictor over
 * the 3 x 3 neighbourhood, codec id "LSOP08".  Tiles need at least 4 rows and 4 columns (else GF_DECLINED, Java null); a singular
 * system is GF_DECLINED too (JAMA throws).  GF_ERR_UNSUPPORTED: more than 16,384 columns or 2^26 or more cells.
 *   residuals: per tile res_stride ints (>= gf_lsop08_residual_count): [2R+2C-5 initialisers | (R-2)(C-2) interior]
 *   coefs:     per tile 16 words: seed, the 8 float32 coefficients as bit patterns, 7 words of 0
 * The container: a 47-byte header (LsHeader.packHeader, never a checksum), then the CodecM32 bytes of the two streams either as two
 * legacy Huffman segments back to back in one bit store (type 0) or as two zlib streams (type 1).  The reference writes type 0
 * only where its body is STRICTLY shorter than the Deflate one.
 *   - gf_lsop08_encode_batch_i32_dev WRITES TYPE 0 ALWAYS: Deflate needs the host's zlib and is not a device-resident operation.  Its
 *     output is the reference's output exactly for the tiles where Huffman is the strictly shorter body.
 *   - the host forms (gf_lsop08_encode_batch_i32, gf_lsop08_encode_i32) give the reference's choice, with the host's zlib at level 6;
 *     types[t] (may be NULL) receives the container type written.  The reference deflates each stream into a buffer of its length +
 *     128 bytes and would write a truncated packing if zlib needed more; such a tile is GF_ERR_UNSUPPORTED here and nothing is written.
 * The decoders take both types and both header revisions and skip a value checksum where bit 7 of the type byte announces one,
 * entirely on the device (the zlib streams by k_inflate).  GF_ERR_FORMAT: a coefficient count other than 8, a type other than 0 or
 * 1, byte counts no encoder can emit; streams that end early: GF_ERR_FORMAT or GF_ERR_BOUNDS.  Nothing outside a packing's bytes is
 * read.  The _dev forms run on the context's stream (as the gf_image_*_dev calls do) and only enqueue; the _dev decode allocates
 * inflate scratch inside the context on first use.                                                                         */
size_t gf_lsop08_residual_count(int n_rows, int n_cols);
size_t gf_lsop08_max_packing(int n_rows, int n_cols);
/* LsOptimalPredictor08.encode: tile -> coefficients + residual streams (d_status: GF_OK / GF_DECLINED per tile) */
gf_status gf_lsop08_predict_dev(gf_context *ctx, int n_rows, int n_cols, size_t n_tiles, const int32_t *d_values,
                                int32_t *d_residuals, size_t res_stride, uint32_t *d_coefs, int32_t *d_status);
/* LsDecoder08.unpackInitializers + unpackInterior: residual streams -> tile.  d_in_status (may be NULL): tiles whose entry is not
 * GF_OK are skipped and keep that status                                                                                      */
gf_status gf_lsop08_reconstruct_dev(gf_context *ctx, int n_rows, int n_cols, size_t n_tiles, const int32_t *d_residuals,
                                    size_t res_stride, const uint32_t *d_coefs, const int32_t *d_in_status, int32_t *d_values,
                                    int32_t *d_status);
/* device-resident batches; d_residuals / d_coefs / d_scratch_status (n_tiles ints) are caller-provided work buffers; d_out: slots of
 * slot_stride bytes (a multiple of 16, 16-byte aligned; gf_lsop08_max_packing always fits; a slot too small: GF_OVERFLOW per tile) */
gf_status gf_lsop08_encode_batch_i32_dev(gf_context *ctx, int codec_index, int n_rows, int n_cols, size_t n_tiles,
                                         const int32_t *d_values, uint8_t *d_out, size_t slot_stride, uint32_t *d_lengths,
                                         int32_t *d_status, int32_t *d_residuals, size_t res_stride, uint32_t *d_coefs,
                                         int32_t *d_scratch_status);
/* d_offsets may be NULL (then packing t starts at t * slot_stride); d_blob 4-byte aligned */
gf_status gf_lsop08_decode_batch_i32_dev(gf_context *ctx, int n_rows, int n_cols, size_t n_tiles, const uint8_t *d_blob,
                                         size_t blob_bytes, const uint64_t *d_offsets, size_t slot_stride,
                                         const uint32_t *d_lengths, int32_t *d_values, int32_t *d_status, int32_t *d_residuals,
                                         size_t res_stride, uint32_t *d_coefs, int32_t *d_scratch_status);
/* host memory */
gf_status gf_lsop08_encode_batch_i32(gf_context *ctx, int codec_index, int n_rows, int n_cols, size_t n_tiles,
                                     const int32_t *values, uint8_t *blob, size_t blob_cap, uint64_t *offsets, uint8_t *types,
                                     int32_t *status);
gf_status gf_lsop08_decode_batch_i32(gf_context *ctx, int n_rows, int n_cols, size_t n_tiles, const uint8_t *blob,
                                     const uint64_t *offsets, int32_t *values, int32_t *status);
gf_status gf_lsop08_encode_i32(gf_context *ctx, int codec_index, int n_rows, int n_cols, const int32_t *values, uint8_t *out,
                               size_t out_cap, size_t *out_len);
gf_status gf_lsop08_decode_i32(gf_context *ctx, int n_rows, int n_cols, const uint8_t *packing, size_t packing_len,
                               int32_t *values);

/* ---- CodecMaster (gvrs/CodecMaster.java:150-169, 195-203): a file's codec list in one batched call ------------------
 * codecs[k] names the k-th entry of the codec list (the standard list of gvrs/GvrsFileSpecification.java:221-230 is
 * {GF_CODEC_HUFFMAN, GF_CODEC_DEFLATE, GF_CODEC_NONE (CodecFloat), GF_CODEC_CANON_HUFFMAN}); k is the codec index written
 * to packing[0].  Encode: every integer codec of the list encodes the batch, per tile the strictly shortest non-null packing
 * wins, list order breaks ties; codec_used[t] = winning index (255: none).  Decode dispatches on packing[0]; an index outside
 * the list is GF_ERR_FORMAT (IOException "Invalid compression-type code").                                                */
#define GF_CODEC_NONE 0
#define GF_CODEC_HUFFMAN 1
#define GF_CODEC_DEFLATE 2
#define GF_CODEC_CANON_HUFFMAN 3
#define GF_CODEC_LSOP12 4
#define GF_CODEC_LSOP08 5   /* in a list: decoded by every call that takes one; encoded by the host forms */
gf_status gf_codec_master_encode_batch_i32(gf_context *ctx, const int *codecs, int n_codecs, int n_rows, int n_cols,
                                           size_t n_tiles, const int32_t *values, uint8_t *blob, size_t blob_cap,
                                           uint64_t *offsets, uint8_t *codec_used, int32_t *status);
gf_status gf_codec_master_decode_batch_i32(gf_context *ctx, const int *codecs, int n_codecs, int n_rows, int n_cols,
                                           size_t n_tiles, const uint8_t *blob, const uint64_t *offsets, int32_t *values,
                                           int32_t *status);

/* ---- tile payloads (gvrs/RasterTile.java:234-256, gvrs/TileElementInt.java:196-219), tiles of one integer element:
 * per tile [int32 LE n][n bytes] = the CodecMaster packing, or the raw little-endian cells when no codec produced a packing or
 * it is not shorter than 4*cells bytes (codec_used[t] = 255).  This is what RecordManager.writeTile stores behind the tile
 * index (gvrs/RecordManager.java:417-431).  Decode treats an element of exactly 4*cells bytes as raw cells.               */
gf_status gf_tile_payload_encode_batch_i32(gf_context *ctx, const int *codecs, int n_codecs, int n_rows, int n_cols,
                                           size_t n_tiles, const int32_t *values, uint8_t *blob, size_t blob_cap,
                                           uint64_t *offsets, uint8_t *codec_used);
gf_status gf_tile_payload_decode_batch_i32(gf_context *ctx, const int *codecs, int n_codecs, int n_rows, int n_cols,
                                           size_t n_tiles, const uint8_t *blob, const uint64_t *offsets, int32_t *values,
                                           int32_t *status);

/* ---- read-ahead: gvrs/TileDecompressionAssistant.java:60-230 and its caller gvrs/RasterTileCache.java:339-426
 * as an N-tile prefetch queue.  The reference's assistant decodes ONE predicted tile on a background thread; this one takes
 * everything that is queued when it wakes up (at most max_batch tiles) and decodes it as one GPU batch through
 * gf_tile_payload_decode_batch_i32, on a context of its own on `device` (the application thread may use its own context
 * at the same time, as the reference's main thread uses its own CodecMaster).
 *   gf_readahead_submit   submitDecompression: `packing` = the element bytes RecordManager.readTilePacking returns (a
 *                         CodecMaster packing, or 4*cells raw little-endian bytes); copied, returns at once
 *   gf_readahead_pending  getPendingTaskCount: queued + in progress
 *   gf_readahead_take     getTilesWithWaitForIndex: waits while wait_index is queued or in progress, then hands over up to
 *                         max_tiles finished tiles (indices[i], values + i*cells, status[i]); the tile waited for comes first.
 *                         Tiles that do not fit stay for the next call.  A wait_index that was never submitted does not wait. */
typedef struct gf_readahead gf_readahead;
gf_status gf_readahead_create(int device, const int *codecs, int n_codecs, int n_rows, int n_cols, size_t max_batch,
                              gf_readahead **ra);
void gf_readahead_destroy(gf_readahead *ra);
gf_status gf_readahead_submit(gf_readahead *ra, int32_t tile_index, const uint8_t *packing, size_t len);
int gf_readahead_pending(gf_readahead *ra);
gf_status gf_readahead_take(gf_readahead *ra, int32_t wait_index, size_t max_tiles, int32_t *indices, int32_t *values,
                            int32_t *status, size_t *n_out);
size_t gf_readahead_cells(gf_readahead *ra);   /* n_rows * n_cols: gf_readahead_take writes that many ints per tile handed over */
void gf_readahead_counters(gf_readahead *ra, uint64_t *n_batches, uint64_t *n_tiles);   /* GPU batches run, tiles decoded */

/* ---- ICompressionDecoder.analyze for CodecHuffman (compress/CodecHuffman.java:172-234, compress/CodecStats.java:49-290):
 * the per-predictor statistics the reference gathers by decoding every packing on the CPU, from a GPU pass that
 * Huffman-decodes the batch and histograms the M32 bytes.  stats[0..4] by predictor code (None, Differencing, Linear,
 * Triangle, DifferencingWithNulls), stats[5] = "All Predictors"; the call ADDS to stats (zero it = clearAnalysisData).
 * The getters of CodecStats are ratios of these sums: bits/symbol = 8 n_bytes / n_symbols, entropy = sum_entropy_m32 /
 * n_m32_counted, ... (CodecStats.java:196-290).  status[t] != GF_OK: the reference's analyze would throw; not counted. */
typedef struct gf_codec_stats {
    int64_t n_tiles;          /* nTilesCounted      */
    int64_t n_bytes;          /* nBytesTotal        : packing bytes - 10 */
    int64_t n_symbols;        /* nSymbolsTotal      : cells */
    int64_t n_bits_overhead;  /* nBitsOverheadTotal : bits of the serialised Huffman tree */
    int64_t n_m32_counted;    /* nM32Counted        */
    int64_t sum_length_m32;   /* sumLengthM32       */
    int64_t sum_observed_m32; /* sumObservedM32     : distinct M32 byte values per tile, summed */
    double sum_entropy_m32;   /* sumEntropyM32      : zero-order entropy of the M32 bytes per tile, summed */
} gf_codec_stats;
gf_status gf_huffman_analyze_batch(gf_context *ctx, int n_rows, int n_cols, size_t n_tiles, const uint8_t *blob,
                                   const uint64_t *offsets, gf_codec_stats *stats, int32_t *status);
/* The same pass with the pair counts behind CodecStats.getH2 (CodecStats.java:63-64, 150-190): pair_counts = six tables of
 * 65536 int64, table k = sB of stats[k], entry (prior << 8) | value counts neighbouring M32 bytes; the call ADDS to them
 * (sA is the column sum of sB).  gf_codec_stats_h2(table) = getH2() of that CodecStats (natural logarithm, as there).   */
gf_status gf_huffman_analyze_batch_h2(gf_context *ctx, int n_rows, int n_cols, size_t n_tiles, const uint8_t *blob,
                                      const uint64_t *offsets, gf_codec_stats *stats, int64_t *pair_counts, int32_t *status);
double gf_codec_stats_h2(const int64_t *pair_table);

/* ---- ICompressionDecoder.analyze for CodecCanonHuffman (compress/canonicalHuffman/CodecCanonHuffman.java:217-324,
 * CanonHuffmanStats.java, CanonicalHuffman.countSymbols / getEntropy / getEscapeBitCounts): the text of every packing is
 * decoded and its symbols counted on the GPU, the sums of CanonHuffmanStats are added to on the host in tile order.
 * stats[0..4] by the predictor byte (PredictorModelType ordinal; 0 holds the uniform form, reported as "Uniform Value"),
 * stats[5] = "All Predictors"; a predictor byte of 5 counts twice there.  escape_counts[6] = escapeBitCounts[1] of the
 * codec: values with 2, 4, 6, 8, 16, 24 escape bits.  Both are ADDED to (zero them = clearAnalysisData).  status[t] != GF_OK
 * (status may be null): the reference's analyze would throw -- nothing counted, except that a predictor byte >= 6 throws
 * only after the tile's escape counts went into escape_counts.  sum_escape_bits leaves the 6-bit class out, as
 * getEscapeBitCountTotal does.                                                                                          */
typedef struct gf_canon_stats {
    int64_t n_tiles;          /* nTilesCounted         */
    int64_t n_bytes;          /* nBytesTotal           : packing bytes - 6 */
    int64_t n_symbols;        /* nSymbolsTotal         : cells */
    int64_t n_bits_overhead;  /* nBitsOverheadTotal    : bits of the code tables (getBitsInCodeTableCount) */
    int64_t n_text_counted;   /* nSymbolsInTextCounted */
    int64_t sum_length;       /* sumLength             : cells */
    int64_t sum_observed;     /* sumObserved           : distinct low bytes of the text per tile, summed */
    double sum_entropy;       /* sumEntropy            : CanonicalHuffman.getEntropy per tile, summed */
    int64_t sum_escape_bits;  /* sumEscapeBits         */
} gf_canon_stats;
gf_status gf_canon_analyze_batch(gf_context *ctx, int n_rows, int n_cols, size_t n_tiles, const uint8_t *blob,
                                 const uint64_t *offsets, gf_canon_stats *stats, int64_t *escape_counts, int32_t *status);

/* ---- tile records (gvrs/RecordManager.java:153-204, 217-262, 386-520; gvrs/TileElementInt.java:196-219,
 * gvrs/TileElementShort.java:211-250; util/GridfourCRC32C.java): what RecordManager.writeTile appends to the file for a
 * tile of one integer-coded element, for a whole batch of dirty tiles in one call (flush()) -- tiles of several elements and of
 * float / int-coded-float elements are read by gf_tile_record_decode_batch_elems[_dev] and written by
 * gf_tile_record_encode_batch_elems[_dev] below:
 *   [int32 LE size, multiple of 8][type 2][0 0 0][int32 tileIndex][int32 n][n element bytes][zeros][CRC-32C | 0]
 * element bytes = CodecMaster packing, or the standard (raw little-endian) form when no codec is listed / produced a
 * packing / it is not shorter (codec_used[t] = 255).  GF_ELEM_SHORT: values are int16, widened with fill_value mapped to
 * INT4_NULL_CODE for the codecs; on decode INT4_NULL_CODE comes back as -32768 (TileElementShort.java:241-243).
 * Reproduces the tile records of the reference's sample files byte for byte (tests/test_gpu_records.py).             */
#define GF_ELEM_INT 0
#define GF_ELEM_SHORT 1
size_t gf_tile_record_max_bytes(int elem_type, int n_rows, int n_cols);
uint32_t gf_crc32c(const uint8_t *data, size_t n);
gf_status gf_tile_record_encode_batch(gf_context *ctx, const int *codecs, int n_codecs, int elem_type, int fill_value,
                                      int n_rows, int n_cols, size_t n_tiles, const int32_t *tile_indices, const void *values,
                                      int checksum_enabled, uint8_t *blob, size_t blob_cap, uint64_t *offsets,
                                      uint8_t *codec_used);
gf_status gf_tile_record_decode_batch(gf_context *ctx, const int *codecs, int n_codecs, int elem_type, int n_rows, int n_cols,
                                      size_t n_tiles, const uint8_t *blob, const uint64_t *offsets, int verify_checksum,
                                      int32_t *tile_indices, void *values, int32_t *status);

/* ---- tile records and mixed-codec packings that already lie in device memory -------------------------------------------
 * The device-resident forms of gf_tile_record_decode_batch and gf_codec_master_decode_batch_i32, for a caller that has read a
 * file region into device memory or whose consumer of the cells is on the GPU: the framing walk, the CRC-32C, the sorting
 * of the packings by the codec their first byte names, the codecs' decoders, the narrowing of shorts and the copy of raw
 * tiles all run on `stream`; nothing is gathered, every decoder reads its packings where they lie in d_blob.
 *   d_blob, d_offsets, d_lengths, d_tile_indices, d_values, d_status are device memory; `codecs` is a host array.
 *   d_blob is 4-byte aligned and readable up to the end of the aligned 4-byte word that holds byte blob_bytes - 1; records
 *   and packings may start at any byte.
 *   gf_tile_record_decode_batch_dev: record t lies in d_blob[d_offsets[t] .. d_offsets[t+1]) (n_tiles + 1 offsets); d_values
 *     is int32 or int16 per elem_type; d_tile_indices may be NULL.
 *   gf_codec_master_decode_batch_i32_dev: packing t = d_lengths[t] bytes at d_blob + d_offsets[t] (n_tiles offsets).
 * Per tile, status, values and tile index are exactly what the host call produces for the same bytes (the values of a tile
 * whose status is not GF_OK are unspecified, as there).  One deliberate difference: the offsets are on the device, so a bad
 * offsets array cannot fail the call as a whole -- a record with d_offsets[t] > d_offsets[t+1] or d_offsets[t+1] > blob_bytes,
 * or a packing with d_offsets[t] + d_lengths[t] > blob_bytes, gets GF_ERR_BOUNDS and nothing of it is read.
 * GF_ERR_ARG, before the device is touched: null pointers, another elem_type, n_rows < 1 or n_cols < 1, a codec kind outside
 * GF_CODEC_NONE .. GF_CODEC_LSOP08, n_codecs > 255 (and, for the codec-master form, n_codecs < 1).  n_tiles == 0 is GF_OK.
 * NOT capture-safe, unlike the other _dev entry points: the host must learn how many tiles each codec has before it can launch
 * the decoders, so these calls SYNCHRONISE `stream` ONCE (a copy of the per-codec counts into page-locked memory) and grow
 * context-owned buffers on demand (the per-record tables; a temporary for the decoded tiles of a batch that mixes codecs,
 * standard-form records or failed records -- a batch in which every record names the same codec is decoded straight into
 * d_values).  Everything before and after the synchronisation is only enqueued.                                          */
gf_status gf_codec_master_decode_batch_i32_dev(gf_context *ctx, void *stream, const int *codecs, int n_codecs, int n_rows,
                                               int n_cols, size_t n_tiles, const uint8_t *d_blob, size_t blob_bytes,
                                               const uint64_t *d_offsets, const uint32_t *d_lengths, int32_t *d_values,
                                               int32_t *d_status);
gf_status gf_tile_record_decode_batch_dev(gf_context *ctx, void *stream, const int *codecs, int n_codecs, int elem_type,
                                          int n_rows, int n_cols, size_t n_tiles, const uint8_t *d_blob, size_t blob_bytes,
                                          const uint64_t *d_offsets, int verify_checksum, int32_t *d_tile_indices,
                                          void *d_values, int32_t *d_status);

/* ---- tile records of several elements, and float / int-coded-float elements, in device memory -------------------------
 * (gvrs/RecordManager.java:492-515, gvrs/RasterTile.java:234-256, gvrs/TileElementFloat.java:222-232,
 * gvrs/TileElementIntCodedFloat.java:172-176, 233-244, gvrs/CodecMaster.java:195-203, 296-304)
 * A tile has n_elems elements, each of one of the four TileElement types; its record holds, behind the tile index, per element
 * [int32 LE n][n bytes] with no padding between elements: element 0's length word is at byte 12 of the record, element e+1's
 * directly behind the bytes of element e.  n == standard size (4*cells for INT, FLOAT and ICF; 2*cells rounded up to 4 for SHORT)
 * means the raw little-endian cells; anything else is a packing whose first byte names an entry of the codec list -- an integer
 * codec for an INT, SHORT or ICF element, a GF_CODEC_NONE entry (the slot of CodecFloat) for a FLOAT element; another entry or an
 * index outside the list is GF_ERR_FORMAT.
 *   elems, codecs and the array d_values itself (n_elems pointers) are HOST memory; d_values[e] points to n_tiles * cells values
 *   of element e in device memory: int32 for INT, int16 for SHORT (INT4_NULL_CODE -> -32768), float32 for FLOAT and ICF.  ICF
 *   delivers code == fill_i ? fill_f : (float)code / scale + offset, single precision, each step rounded once.
 *   d_status is element-major, d_status[e * n_tiles + t]; d_tile_indices may be NULL.  d_blob, d_offsets, record placement, the
 *   bounds rule for a bad d_offsets entry and "synchronises `stream` once, not capture-safe" are exactly as for
 *   gf_tile_record_decode_batch_dev; one partition, one count read-back and one synchronisation serve all elements, and every
 *   codec's decoder is launched once for the packings of all elements.
 * Per record: the record head, the type byte and (verify_checksum) the CRC-32C are judged as gf_tile_record_decode_batch_dev judges
 * them, in its order, and a failure there is the status of EVERY element of the record.  An element whose length word or bytes
 * do not fit the record (position + 4 + n > size) is GF_ERR_BOUNDS, and so is every element behind it, which cannot be located;
 * the elements in front of it are decoded and keep their own status.  A decoder's verdict on one element does not change the
 * other elements of the record.  The reference reads a tile as a whole and would throw: A TILE IS GOOD IFF ALL ITS ELEMENT
 * STATUSES ARE GF_OK.  With n_elems == 1 and type INT or SHORT the call answers exactly as gf_tile_record_decode_batch_dev.
 * GF_ERR_ARG, before the device is touched: null pointers (ctx, codecs with n_codecs > 0, elems, d_blob, d_offsets, d_values or
 * one of its entries, d_status), n_elems < 1 or > GF_MAX_ELEMS, a type outside 0..3, an ICF scale that is 0 or NaN, a codec kind
 * outside GF_CODEC_NONE .. GF_CODEC_LSOP08, n_codecs > 255, n_rows < 1, n_cols < 1, an unaligned d_blob.  GF_ERR_UNSUPPORTED:
 * n_elems * n_tiles > 0x7fffffff.  n_tiles == 0 is GF_OK.
 * gf_tile_record_decode_batch_elems is the same call for bytes in host memory (values[e], tile_indices, status: host arrays;
 * offsets[n_tiles] bytes of blob are read): it stages blob and offsets into buffers of the context, calls the device form on
 * the context's stream and copies values, indices and statuses back.  It is NOT pipelined as gf_tile_record_decode_batch is: a
 * convenience for ctypes / JNI callers, not a rate.                                                                         */
#define GF_ELEM_FLOAT 2   /* TileElementFloat: float32 cells; a packing is a CodecFloat packing */
#define GF_ELEM_ICF   3   /* TileElementIntCodedFloat: stored exactly as GF_ELEM_INT, delivered as float32 */
#define GF_MAX_ELEMS 16
typedef struct gf_elem_spec {
    int32_t type;      /* GF_ELEM_*                                                      */
    int32_t fill_i;    /* ICF: fillValueI, the stored code of "no data"; INT, SHORT: the fill value of a block read, else ignored */
    float scale;       /* ICF: value = code / scale + offset (TileElementIntCodedFloat.java:172-176) */
    float offset;
    float fill_f;      /* ICF: what a cell equal to fill_i is delivered as (may be NaN); FLOAT, ICF: the fill value of a block read */
} gf_elem_spec;
gf_status gf_tile_record_decode_batch_elems_dev(gf_context *ctx, void *stream, const int *codecs, int n_codecs,
                                                const gf_elem_spec *elems, int n_elems, int n_rows, int n_cols, size_t n_tiles,
                                                const uint8_t *d_blob, size_t blob_bytes, const uint64_t *d_offsets,
                                                int verify_checksum, int32_t *d_tile_indices, void *const *d_values,
                                                int32_t *d_status);
gf_status gf_tile_record_decode_batch_elems(gf_context *ctx, const int *codecs, int n_codecs, const gf_elem_spec *elems,
                                            int n_elems, int n_rows, int n_cols, size_t n_tiles, const uint8_t *blob,
                                            const uint64_t *offsets, int verify_checksum, int32_t *tile_indices,
                                            void *const *values, int32_t *status);

/* ---- tile records of several elements WRITTEN, in device memory: framing and CRC-32C on the GPU -----------------------------
 * (gvrs/RecordManager.java:386-490 writeTile, gvrs/RasterTile.java:234-256 getCompressedPacking, gvrs/TileElementInt.java:196-206,
 * gvrs/TileElementShort.java:100-110, 211-229, gvrs/TileElementFloat.java:209-219, gvrs/CodecMaster.java:150-169, 261-280)
 * What RecordManager.writeTile appends to the file for tiles of n_elems elements, the inverse of gf_tile_record_decode_batch_elems[_dev]:
 *   [int32 LE size, multiple of 8][type 2][0 0 0][int32 tileIndex] { [int32 n][n bytes] per element, no padding between } [zeros][CRC-32C | 0]
 *   size = multipleOf8(4 + sum(4 + n_e) + 12).  Element bytes = the CodecMaster packing (the strictly shortest non-null packing over
 *   the list, list order on ties) or, when no codec produced one or it is not shorter than the standard size, the standard form:
 *   the little-endian cells, 4 * cells bytes for INT, FLOAT and ICF, 2 * cells rounded up to a multiple of 4 for SHORT (the two
 *   extra bytes zero).  A SHORT element goes to the codecs as int32 with cells equal to (int16)fill_i mapped to INT4_NULL_CODE.
 *   hasValidData() and the free-space list are the record manager's business: the caller lists the tiles it wants written.
 *   elems, codecs and the array d_values itself (n_elems pointers) are HOST memory; d_values[e] points to n_tiles * cells items of
 *   element e in device memory, 4-byte aligned: int32 for INT, int16 for SHORT, float32 for FLOAT (cells move as bits) and, for
 *   ICF, the int32 CODES the tile holds -- the float-to-code conversion is TileElementIntCodedFloat.setValue, a tile-cache
 *   operation with range checks that throw, not part of writeTile (gf_block_write_elems_dev below does it).  The d_values[e] of a SHORT element must be readable to the
 *   end of the aligned 4-byte word that holds its last cell (the kernels read whole aligned words).
 *   d_offsets[n_tiles + 1]: record t is d_blob[d_offsets[t] .. d_offsets[t+1]), d_offsets[0] = 0.  d_blob is 8-byte aligned.
 *   d_codec_used (may be NULL) is element-major, d_codec_used[e * n_tiles + t]: the winning list index, or 255 for the standard
 *   form.  d_status[t]: GF_OK, or the first negative status of an encoder that failed on one of the tile's elements (the Java
 *   encoder would throw; unlike gf_codec_master_encode_batch_i32 the failure is not forgiven when another codec packs the
 *   tile): such a record has length 0 and nothing of it is written.  A candidate that is GF_DECLINED, GF_OVERFLOW (the slots are
 *   at least as long as the standard form) or not shorter than the standard size simply loses.
 *   Capacity as for gf_compact_dev: a record that would end behind blob_cap is skipped whole, d_offsets[n_tiles] > blob_cap tells
 *   the caller; no byte at or behind blob_cap is written, and every byte of a written record is written exactly once per call.
 * The device form takes lists of GF_CODEC_HUFFMAN and GF_CODEC_CANON_HUFFMAN entries, and GF_CODEC_NONE entries as long as no
 * element is FLOAT; n_codecs == 0 is "compression disabled": everything in standard form.  GF_ERR_UNSUPPORTED, from the arguments
 * alone: a list with GF_CODEC_DEFLATE, GF_CODEC_LSOP12 or GF_CODEC_LSOP08 (their containers' choice needs zlib), a GF_CODEC_NONE
 * entry together with a FLOAT element (CodecFloat's zlib streams); and for both forms n_elems * n_tiles > 0x7fffffff, 2^28 or more
 * cells in a tile, a record that could exceed 0x7fffffff bytes (gf_tile_record_max_bytes_elems).
 * GF_ERR_ARG, before the device is touched: null pointers (ctx, codecs with n_codecs > 0, elems, tile indices, d_values or one of
 * its entries, d_blob, d_offsets, d_status), n_elems < 1 or > GF_MAX_ELEMS, a type outside 0..3, an ICF scale that is 0 or NaN, a
 * SHORT fill_i outside int16, a codec kind outside GF_CODEC_NONE .. GF_CODEC_LSOP08, n_codecs > 255, n_rows < 1, n_cols < 1, a
 * d_blob that is not 8-byte or a d_values[e] that is not 4-byte aligned.  n_tiles == 0 is GF_OK.
 * The device form ONLY ENQUEUES on `stream` and never synchronises it: every codec runs on every tile and the layout is a scan, so
 * nothing has to come back to the host.  It grows buffers of the context on demand (candidate slots, their lengths and statuses,
 * widened SHORT cells: hipMalloc / hipFree); a second call with the same or smaller arguments allocates nothing.  Whether it can be
 * captured into a hipGraph after such a warm-up call has NOT been tested and is not claimed.
 * gf_tile_record_encode_batch_elems is the call for host memory and takes any list.  A list the device form accepts is staged into
 * buffers of the context and sent through the device form (not pipelined); any other list is encoded element by element with the
 * host entry points (gf_codec_master_encode_batch_i32; gf_float_encode_batch_f32 under the index of the list's first GF_CODEC_NONE
 * entry, zlib level 6 as the reference's sample files were written) and framed on host threads.  It returns the first negative
 * per-tile status as its own, and GF_ERR_CAPACITY with offsets[n_tiles] filled in when blob_cap is too small, as
 * gf_tile_record_encode_batch does.  gf_tile_record_max_bytes_elems: the size of a record whose elements are all in standard form
 * (0 for arguments the calls refuse).                                                                                          */
size_t gf_tile_record_max_bytes_elems(const gf_elem_spec *elems, int n_elems, int n_rows, int n_cols);
gf_status gf_tile_record_encode_batch_elems_dev(gf_context *ctx, void *stream, const int *codecs, int n_codecs,
                                                const gf_elem_spec *elems, int n_elems, int n_rows, int n_cols, size_t n_tiles,
                                                const int32_t *d_tile_indices, const void *const *d_values, int checksum_enabled,
                                                uint8_t *d_blob, size_t blob_cap, uint64_t *d_offsets, uint8_t *d_codec_used,
                                                int32_t *d_status);
gf_status gf_tile_record_encode_batch_elems(gf_context *ctx, const int *codecs, int n_codecs, const gf_elem_spec *elems,
                                            int n_elems, int n_rows, int n_cols, size_t n_tiles, const int32_t *tile_indices,
                                            const void *const *values, int checksum_enabled, uint8_t *blob, size_t blob_cap,
                                            uint64_t *offsets, uint8_t *codec_used);

/* ---- grid blocks: a rectangle of the raster read from tiles, and a raster cut into tiles, in device memory ------------------
 * (gvrs/GvrsElement.java:298-404 readBlock / readBlockInt, gvrs/TileAccessIndices.java:79-88, gvrs/GvrsFileSpecification.java:423-424)
 * The grid is cut into tiles of n_rows_tile x n_cols_tile cells: ceil(n_cols_grid / n_cols_tile) tiles across, ceil(n_rows_grid /
 * n_rows_tile) down, tile index = tileRow * nColsOfTiles + tileCol; the tiles of the last tile row and column reach beyond the
 * grid.  A gf_rect is in grid coordinates and lies wholly inside the grid.  A block is the rectangle's cells, row-major, n_rows x
 * n_cols items of the element's delivered type: 2 bytes for GF_ELEM_SHORT, 4 for INT, FLOAT and ICF.  Cells move as bits (NaN
 * payloads and -0.0 survive); fill_bits is the fill value's bit pattern (the low 16 bits for SHORT).  All cell counts and
 * addresses are 64 bits wide on host and device.
 *   gf_block_from_tiles_dev: d_tiles holds n_tiles decoded tiles (tile j = cells items at d_tiles + j * cells), d_tile_indices[j]
 *   the tile index of each, in any order.  Every cell of d_block is written exactly once: from the tile that covers it, or with
 *   the fill value where no listed tile does or d_tile_status (may be NULL) of that tile is not GF_OK.  An index that is
 *   negative, beyond the grid's tiles or outside the rectangle's tiles places nothing; of two entries with one index the later
 *   one wins, whatever the timing.  Never synchronises and allocates only when the context's slot table has to grow (call it
 *   once before a capture): safe for hipGraph capture.  The slot table is ONE buffer of the context, written and read by the work
 *   this call enqueues: the gathers of one context (this call and the two record forms) must all be enqueued on one stream, or
 *   be ordered by the caller; and a recorded graph holds the table's address, so it is invalid once a later gather of the
 *   context with a larger rectangle of tiles has made the table grow (it never shrinks: gather the largest rectangle first).
 *   gf_tiles_from_block_dev, the inverse: d_block is the rectangle's cells; for each listed tile (tile j of d_tiles is tile
 *   d_tile_indices[j] of the grid) every cell whose grid coordinate lies inside the rectangle takes the block's value; every
 *   other cell, those beyond the grid included, takes the fill value when keep_outside == 0 and is left untouched otherwise (a
 *   block written into existing tiles).  d_status (may be NULL): GF_OK, or GF_ERR_BOUNDS for an index outside the grid's tiles,
 *   of which nothing is written.  Capture-safe.
 *   gf_block_read_elems_dev: gf_tile_record_decode_batch_elems_dev into a temporary of the context, then the gather: d_blocks
 *   (a HOST array of n_elems device pointers) receives one block per element in its delivered type (no int-to-float conversion
 *   as in readBlock on an integer element).  Records come in any order; records of tiles that do not touch the rectangle are
 *   decoded and ignored.  d_status is exactly what gf_tile_record_decode_batch_elems_dev reports; the cells of a failed element
 *   read as fill (the reference would throw: THE BLOCK IS GOOD IFF EVERY STATUS IS GF_OK).  Fill per element: fill_i for INT
 *   and SHORT (outside int16 for a SHORT: GF_ERR_ARG), fill_f for FLOAT and ICF.  Synchronises `stream` once, not capture-safe.
 *   With n_records == 0 the blocks are all fill.  gf_block_read_elems is the same for bytes, blocks and statuses in host memory,
 *   staged as gf_tile_record_decode_batch_elems stages; only the blocks and the statuses are copied back.
 * GF_ERR_ARG, before the context or a device is looked at: null pointers, one of the eight numbers < 1 (row0 / col0 < 0), a
 * rectangle not wholly inside the grid (the reference throws), an elem_type outside GF_ELEM_*, and for the two record forms
 * whatever gf_tile_record_decode_batch_elems[_dev] rejects (n_rows, n_cols: the tile's).  GF_ERR_UNSUPPORTED: more than 0x7fffffff
 * tiles in the grid or entries in a list, 2^28 or more cells in a tile.                                                          */
typedef struct gf_grid_spec { int32_t n_rows_grid, n_cols_grid, n_rows_tile, n_cols_tile; } gf_grid_spec;
typedef struct gf_rect      { int32_t row0, col0, n_rows, n_cols; } gf_rect;   /* grid coordinates */
gf_status gf_block_from_tiles_dev(gf_context *ctx, void *stream, const gf_grid_spec *grid, const gf_rect *rect, int elem_type,
                                  uint32_t fill_bits, size_t n_tiles, const int32_t *d_tile_indices, const int32_t *d_tile_status,
                                  const void *d_tiles, void *d_block);
gf_status gf_tiles_from_block_dev(gf_context *ctx, void *stream, const gf_grid_spec *grid, const gf_rect *rect, int elem_type,
                                  uint32_t fill_bits, int keep_outside, const void *d_block, size_t n_tiles,
                                  const int32_t *d_tile_indices, void *d_tiles, int32_t *d_status);
gf_status gf_block_read_elems_dev(gf_context *ctx, void *stream, const int *codecs, int n_codecs, const gf_elem_spec *elems,
                                  int n_elems, const gf_grid_spec *grid, const gf_rect *rect, size_t n_records,
                                  const uint8_t *d_blob, size_t blob_bytes, const uint64_t *d_offsets, int verify_checksum,
                                  void *const *d_blocks, int32_t *d_status);
gf_status gf_block_read_elems(gf_context *ctx, const int *codecs, int n_codecs, const gf_elem_spec *elems, int n_elems,
                              const gf_grid_spec *grid, const gf_rect *rect, size_t n_records, const uint8_t *blob,
                              const uint64_t *offsets, int verify_checksum, void *const *blocks, int32_t *status);

/* ---- a grid block INTERPOLATED: B-spline value, derivatives and unit normal at a batch of grid coordinates ---------------------
 * (gvrs/GvrsInterpolatorBSpline.java:327-334 zInterpGrid, :283-304 zNormalGrid, :374-445 loadSamples, :447-484 loadWrappingSamples,
 * :307-314 blockLimit; interpolation/InterpolatorBSpline.java:159-379 interpolate; InterpolationResult.java:129-139 getUnitNormal)
 * For every query point (row, column), doubles in GRID coordinates, the reference reads the 4 x 4 block of cells around it and
 * evaluates a bicubic B-spline on the 16 samples.  These calls do the same for a batch of points over a block that lies in device
 * memory (what gf_block_read_elems_dev delivers: d_block holds the rectangle spec->block, row-major, in the element's delivered
 * type, aligned to its item size), BIT FOR BIT: the window is chosen as loadSamples / loadWrappingSamples choose it, the evaluation is
 * interpolate(1.0 + v, 1.0 + u, 4, 4, z, row_spacing, column_spacing, target) with its own floor and outer-band adjustments, every
 * operation in the reference's order, in double, without fused multiply-add.
 *   z is what zInterpGrid returns; with target GF_INTERP_FIRST zx, zy and normal are what zNormalGrid's result holds (normal:
 *   getUnitNormal, 3 doubles per point, interleaved); with GF_INTERP_SECOND zxx, zxy (= zyx), zyy as well.  An output array the
 *   target does not compute is filled with NaN, as the reference sets those fields (InterpolatorBSpline.java:295-300, :372-375).
 *   SAMPLES: FLOAT and ICF cells are used as they are; an INT or SHORT cell equal to fill_i reads as NaN, any other as (float) cell
 *   (TileElementInt.java:150-156, TileElementShort.java:167-173), widened to double (InterpolatorBSpline.java:231-249).
 *   wrap: 0, or what GvrsFileSpecification reports: 1 doGeographicCoordinatesWrapLongitude, 2 ... and ...BracketLongitude
 *   (nColsForWrap = n_cols_grid - 1, GvrsInterpolatorBSpline.java:139-143).  The fringes are GvrsFileSpecification.java:437-440.
 *   NOT DONE BY THESE CALLS: mapModelToGridPoint / mapGeographicToGridPoint, and zNormal's column spacing cos(latitude) * du
 *   with its dx < 1 -> 1 clamp (:291-299).  Both are the section "GVRS files queried at COORDINATES" below: gf_file_map_points
 *   gives rows, columns and the column spacing per point for these calls (d_col_spacing; per lattice row: d_col_spacing_rows;
 *   NULL: spec->col_spacing for all), and gf_file_interp_coords_dev does mapping, spacing and interpolation in one.
 *   LATTICE FORM: point (i, j), 0 <= i < n_rows, 0 <= j < n_cols, has row = row0 + (double)i * row_step, col = col0 + (double)j *
 *   col_step, one product and one sum, each rounded once; outputs are row-major n_rows x n_cols.  It gives the bits the points
 *   form gives for those coordinates (one kernel serves both).
 *   PER-POINT STATUS (out->status, may be NULL), first match: GF_ERR_ARG a NaN coordinate (interpolate throws); GF_DECLINED outside
 *   the fringe (the reference returns NaN / a nullified result); GF_ERR_ARG a wrapped window the reference's readBlock rejects
 *   (n1 < 1 or n2 < 1, GvrsElement.java:457-460); GF_ERR_BOUNDS the 4 x 4 window, or either part of a wrapped one, is not wholly
 *   inside spec->block; GF_ERR_ARG a zero column spacing for the point with target >= GF_INTERP_FIRST (:304-307); else GF_OK.
 *   With any status other than GF_OK every output array passed receives NaN for that point.  Every output item is written
 *   exactly once.
 * The device forms ONLY ENQUEUE on `stream` (NULL: the context's), allocate nothing, never synchronise and are safe for hipGraph
 * capture.  gf_block_interp_points is the same for block, coordinates and outputs in host memory, staged through a buffer of the
 * context: a convenience, not a rate.
 * GF_ERR_ARG, before the context or a device is looked at: a NULL ctx, spec, block, out or out->z; NULL coordinate arrays with
 * n_points > 0; a grid under 4 x 4 (the reference's constructor throws, :113-116); a block not wholly inside the grid or under
 * 4 x 4; an elem_type, wrap or target out of range; a SHORT fill_i outside int16; with target >= GF_INTERP_FIRST a zero
 * row_spacing, or a zero col_spacing without per-point / per-row spacings; normal with target GF_INTERP_VALUE; a NULL lattice
 * or a lattice count below 1.  GF_ERR_UNSUPPORTED: a lattice of 2^63 or more points.  n_points == 0: GF_OK.                      */
#define GF_INTERP_VALUE 0
#define GF_INTERP_FIRST 1
#define GF_INTERP_SECOND 2
typedef struct gf_interp_spec {
    int32_t n_rows_grid, n_cols_grid;   /* the raster; each >= 4                                                       */
    gf_rect block;                      /* the rectangle of the raster that d_block holds, inside the grid, >= 4 x 4   */
    int32_t elem_type, fill_i;          /* GF_ELEM_*; INT, SHORT: a cell equal to fill_i reads as NaN                  */
    int32_t wrap;                       /* 0 none; 1 wraps longitude; 2 wraps and brackets longitude                   */
    int32_t target;                     /* GF_INTERP_*                                                                 */
    double row_spacing, col_spacing;    /* dv, du; non-zero when target >= GF_INTERP_FIRST                             */
    double row_fringe0, row_fringe1, col_fringe0, col_fringe1;
} gf_interp_spec;
typedef struct gf_interp_out {          /* arrays of one item per point; any may be NULL except z                      */
    double *z, *zx, *zy, *zxx, *zxy, *zyy;
    double *normal;                     /* 3 per point, interleaved; needs target >= GF_INTERP_FIRST                   */
    int32_t *status;
} gf_interp_out;
typedef struct gf_interp_lattice { double row0, col0, row_step, col_step; int64_t n_rows, n_cols; } gf_interp_lattice;
gf_status gf_block_interp_points_dev(gf_context *ctx, void *stream, const gf_interp_spec *spec, const void *d_block, size_t n_points,
                                     const double *d_rows, const double *d_cols, const double *d_col_spacing,
                                     const gf_interp_out *out);
gf_status gf_block_interp_lattice_dev(gf_context *ctx, void *stream, const gf_interp_spec *spec, const void *d_block,
                                      const gf_interp_lattice *lattice, const double *d_col_spacing_rows, const gf_interp_out *out);
gf_status gf_block_interp_points(gf_context *ctx, const gf_interp_spec *spec, const void *block, size_t n_points, const double *rows,
                                 const double *cols, const double *col_spacing, const gf_interp_out *out);

/* ---- a grid block RENDERED: one ARGB word per cell or per pixel, through a colour palette and a shaded relief ---------------------
 * (imaging/palette/ColorPaletteTable.java:162-253 the constructor, :395-456 getArgb, :481-541 getArgbWithShade, :567-598
 * getArgbUnlimitedRange[WithShade]; ColorPaletteRecord.java:176-182 compareTo; ColorPaletteRecordRGB.java:72-121;
 * ColorPaletteRecordHSV.java:95-194; the illumination model of demo/src/main/java/org/gridfour/demo/globalDEM/ExtractData.java:
 * 394-419 and demo/geoTiff/DemoCOG.java:405-441)
 * What the reference's demos do per pixel after interpolating -- a shade from the surface's first derivatives, a colour from a
 * palette, both in one int 0xAARRGGBB -- over a block that lies in device memory, BIT FOR BIT: doubles in the reference's operation
 * order, no fused multiply-add, Java's (int) conversions, java.util.Arrays.binarySearch(double[], double) as the JDK walks it (with
 * equal keys the probe sequence decides, -0.0 sorts below a key 0.0, NaN above everything), 32-bit shifts and ORs for the word (a
 * shade outside 0..1 gives the bits Java gives), java.awt.Color.HSBtoRGB in float32 for HSV records.
 *   PALETTE.  gf_palette_create does on the host what the table's constructor does: it sorts the records by (range0, range1) in
 *   Double.compare's order (-0.0 < 0.0), stably; keys[i] = range0 of record i; hingeIndex = the first record whose range0 ==
 *   hinge_value; per RGB record deltaR/G/B, per HSV record deltaS, deltaV, deltaH (|h1 - h0| < 1.0e-6 -> 0, else brought into
 *   (-180, 180], 0 -> 360) and wrapAround.  It uploads one packed table, allocates and synchronises; rendering does neither.  The
 *   palette belongs to the context's device, is read-only afterwards and may serve any number of calls; gf_palette_destroy frees
 *   it (NULL is allowed).  normalized / range_min / range_max / hinge / hinge_value are the second constructor's arguments
 *   (normalized == 0 and hinge == 0: the first constructor); argb_for_null is Color.getRGB() of colorForNull, 0 without one.
 *   The library does not parse palette files.
 *   DEVIATION: normalized && hinge with the hinge on the FIRST record is refused: the reference's constructor accepts it and then
 *   indexes records[-1] on the first z below the hinge (:409).
 *   gf_palette_create: GF_ERR_ARG, before the context or a device is looked at: a NULL spec, records, out or ctx; n_records < 1;
 *   a record with !(range0 <= range1) (NaN included); a model other than GF_PALETTE_RGB / GF_PALETTE_HSV; an RGB channel outside
 *   0..255; hinge with a hinge_value that equals no range0 (the constructor throws); the deviation above.  GF_ERR_UNSUPPORTED:
 *   more than GF_PALETTE_MAX_RECORDS records.
 *   LOOKUP.  z -> the normalised / hinge remapping as written (:405-420), the binary search on the keys, index == -1 -> the null
 *   colour, else the record found or the one before the insertion point when its range1 >= z, else the null colour; the record
 *   interpolates between its two colours (t clamped by the two comparisons; a NaN t, range0 == range1, yields channel 0).  NaN and
 *   +-infinity give the null colour.  flags & GF_RENDER_UNLIMITED: getArgbUnlimitedRange (z clamped to records[0].range0 ..
 *   records[n - 1].range1 first); with a shade the WithShade forms.
 *   gf_block_render_cells_dev: n_cells cells (int32 / int16 / float32 as elem_type says, aligned to the item; INT and SHORT: a cell
 *   equal to fill_i reads as NaN, any other as (float) cell, FLOAT and ICF as they are, widened to double: the interpolator's
 *   samples) -> d_argb[n_cells] (4-byte aligned).  d_shade (may be NULL, 8-byte aligned): one double per cell.  elem_type
 *   GF_RENDER_Z, this call alone: d_cells holds doubles, looked up as they are -- z as gf_block_interp_*_dev delivers it, with a
 *   shade array of the caller's: the unfused form of the lattice call below, the same words.
 *   gf_block_render_lattice_dev: spec, d_block and lattice as gf_block_interp_lattice_dev takes them; per pixel the sixteen samples
 *   and the interpolator's own sums (the same functions: z, zx, zy are the bits gf_block_interp_lattice_dev delivers), then
 *     nx = zx * x_gain; ny = zy * y_gain; s = sqrt(nx * nx + ny * ny + 1); nx /= s; ny /= s; nz = 1 / s;
 *     dot = nx * sun[0] + ny * sun[1] + nz * sun[2]; shade = ambient; if (dot > 0) shade = dot * (1 - ambient) + ambient;
 *   and the lookup of z with that shade.  ExtractData: x_gain = -steepen, y_gain = +steepen; DemoCOG: both -steepen.  The sun
 *   vector comes from the caller (libm's sine and cosine do not reproduce bit for bit).  light == NULL: no shade, the value alone
 *   is evaluated and looked up without shade.  spec->target is checked and otherwise ignored: first derivatives are evaluated
 *   with a light, the value alone without.  out->argb [n], out->shade [n] (the shade, needs a light) and out->status [n] (the
 *   interpolator's per-point status) may each be NULL, but not both argb and shade.  A pixel whose status is not GF_OK has NaN z,
 *   zx and zy by the interpolator's rule and goes the same way: the null colour, the ambient shade.
 *   gf_block_render_points_dev: the lane-per-point form.  lattice != NULL: a lattice whose column spacing differs per ROW
 *   (d_col_spacing: n_rows entries; ExtractData's xScale = yScale * cos(latitude)); d_rows, d_cols must be NULL.  lattice == NULL:
 *   n_points free points d_rows, d_cols, d_col_spacing per point.  d_col_spacing == NULL: spec->col_spacing.  A zero spacing gives
 *   the pixel GF_ERR_ARG, as there.
 *   gf_block_render_lattice: block and outputs in host memory, staged through a buffer of the context; it synchronises: a
 *   convenience, not a rate.
 * The device forms ONLY ENQUEUE on `stream` (NULL: the context's), allocate nothing, never synchronise and are safe for hipGraph
 * capture.  Every output item is written exactly once and nothing else is written.
 * GF_ERR_ARG, before the context or a device is looked at: what gf_block_interp_*_dev reject of ctx, spec, block, lattice and
 * coordinate arrays (with a light: the zero-spacing rules of target GF_INTERP_FIRST); a NULL palette; a NULL out, or out->argb and
 * out->shade both NULL; out->shade without a light; flags other than GF_RENDER_UNLIMITED; both a lattice and coordinate arrays;
 * cells form: an elem_type outside GF_ELEM_INT .. GF_RENDER_Z, a SHORT fill_i outside int16, NULL d_cells or d_argb with n_cells > 0, a misaligned pointer.
 * GF_ERR_UNSUPPORTED: a lattice of 2^63 or more points, more than 2^48 cells.  n_points == 0, n_cells == 0: GF_OK.  A palette of
 * another device than the context's: GF_ERR_ARG.                                                                               */
#define GF_PALETTE_RGB 0
#define GF_PALETTE_HSV 1
#define GF_PALETTE_MAX_RECORDS 256
#define GF_RENDER_UNLIMITED 1
#define GF_RENDER_Z 4                   /* gf_block_render_cells_dev: elem_type of double cells                        */
typedef struct gf_palette gf_palette;
typedef struct gf_palette_record {
    double range0, range1;              /* range0 <= range1                                                            */
    int32_t model;                      /* GF_PALETTE_RGB, GF_PALETTE_HSV                                              */
    int32_t rgb0[3], rgb1[3];           /* RGB: red, green, blue at range0 / range1, each 0..255                       */
    int32_t reserved;
    double hsv0[3], hsv1[3];            /* HSV: hue (degrees), saturation, value at range0 / range1                    */
} gf_palette_record;
typedef struct gf_palette_spec {
    const gf_palette_record *records;
    int32_t n_records;                  /* 1 .. GF_PALETTE_MAX_RECORDS                                                 */
    uint32_t argb_for_null;
    int32_t normalized, hinge;          /* booleans                                                                    */
    double range_min, range_max;        /* normalizedRangeMin / Max (normalized)                                       */
    double hinge_value;                 /* (hinge) the range0 of a record                                              */
} gf_palette_spec;
typedef struct gf_render_light { double x_gain, y_gain, sun[3], ambient; } gf_render_light;
typedef struct gf_render_out { int32_t *argb; double *shade; int32_t *status; } gf_render_out;
gf_status gf_palette_create(gf_context *ctx, const gf_palette_spec *spec, gf_palette **out);
void gf_palette_destroy(gf_palette *palette);
gf_status gf_block_render_cells_dev(gf_context *ctx, void *stream, const gf_palette *palette, int flags, int elem_type, int32_t fill_i,
                                    const void *d_cells, size_t n_cells, const double *d_shade, int32_t *d_argb);
gf_status gf_block_render_lattice_dev(gf_context *ctx, void *stream, const gf_interp_spec *spec, const void *d_block,
                                      const gf_interp_lattice *lattice, const gf_palette *palette, const gf_render_light *light,
                                      int flags, const gf_render_out *out);
gf_status gf_block_render_points_dev(gf_context *ctx, void *stream, const gf_interp_spec *spec, const void *d_block,
                                     const gf_interp_lattice *lattice, size_t n_points, const double *d_rows, const double *d_cols,
                                     const double *d_col_spacing, const gf_palette *palette, const gf_render_light *light, int flags,
                                     const gf_render_out *out);
gf_status gf_block_render_lattice(gf_context *ctx, const gf_interp_spec *spec, const void *block, const gf_interp_lattice *lattice,
                                  const gf_palette *palette, const gf_render_light *light, int flags, const gf_render_out *out);

/* ---- a grid block DOWNSAMPLED: the box average by an integer factor, in device memory -------------------------------------------
 * (demo/src/main/java/org/gridfour/demo/globalDEM/ExampleDownsample.java:164-210 the loop, :228-239 makeSpec's grid size)
 * The coarser copy of a raster that the reference's ExampleDownsample writes -- an overview or pyramid level -- computed over a block
 * that lies in device memory, bit for bit: output cell (i, j) of the coarse grid covers source rows i * f .. i * f + f - 1 and
 * columns j * f .. j * f + f - 1, visited in row-major order; the coarse grid has floor(rows / f) x floor(cols / f) cells.
 *   INT, SHORT: a window with ANY cell equal to fill_i gives fill_i (the reference leaves the cell unpopulated); else the cells are
 *   summed as Java ints (wrap-around), avg = (double) sum / (f * f), the result (int) Math.floor(avg + 0.5).  No range check is made
 *   (that is gf_block_write_elems[_dev]'s part); a SHORT's result always fits int16.
 *   FLOAT: float sum = 0; sum += cell, one float32 rounding per addition in row-major order; the result sum / (float)(f * f).  The
 *   fill gets no special treatment: a NaN fill propagates, any other is averaged in.  f = 1 turns -0.0 into +0.0, +inf and -inf in
 *   one window give NaN, subnormals are not flushed.
 *   ICF: the reference averages the CODES of an int-coded float (readBlockInt, fillValueI), never the float values, and a block read
 *   under GF_ELEM_ICF holds float values: the two plain forms refuse GF_ELEM_ICF with GF_ERR_UNSUPPORTED.  Read the element as
 *   GF_ELEM_INT with fill_i = fillValueI and downsample that; gf_block_read_downsampled_elems[_dev] does so by itself.
 *   gf_block_downsample_rect (host arithmetic only): block is the rectangle of the SOURCE grid an input block holds; out is the
 *   rectangle, in the COARSE grid's coordinates, of the output cells whose whole window lies inside block: row0' = ceil(row0 / f),
 *   n_rows' = floor((row0 + n_rows) / f) - row0', the same for columns.  An empty result has n_rows' = 0 or n_cols' = 0 and is GF_OK.
 *   A block need not start on a multiple of f: a caller working through a raster in strips gets the cells of one call on the whole.
 *   gf_block_downsample_elems_dev: elems[n_elems] (type and fill_i are looked at); d_blocks and d_out are HOST arrays of n_elems
 *   device pointers, each 4-byte aligned.  d_blocks[e] is the block `block` of element e as gf_block_read_elems_dev delivers it:
 *   row-major, int32 / int16 / float32 (a SHORT block must be readable to the end of the aligned 4-byte word that holds its last
 *   cell; otherwise nothing outside the blocks is read).  d_out[e] receives n_rows' x n_cols' items of the same type, row-major:
 *   every item is written exactly once and nothing else is written.  An empty output rectangle is GF_OK and touches nothing.  The
 *   call ONLY ENQUEUES on `stream` (NULL: the context's), one launch per element: it never synchronises, never allocates, and is
 *   safe for hipGraph capture.  gf_block_downsample_elems is the same for blocks and outputs in host memory, staged through a
 *   buffer of the context on the context's stream; it synchronises.
 *   gf_block_read_downsampled_elems_dev: gf_block_read_elems_dev's arguments plus factor: tile records in, one COARSE block per
 *   element out, for the rectangle gf_block_downsample_rect(rect, factor) gives.  The full-resolution blocks live in a temporary
 *   of the context that grows on demand; then the kernels above run.  d_status is exactly the block read's: the result is good iff
 *   every status is GF_OK (a missing tile and a failed record read as fill).  A GF_ELEM_ICF element IS accepted here: it is read
 *   as INT on fill_i, averaged on its codes and delivered as int32 codes -- written back as a GF_ELEM_INT element these are the
 *   bytes of an ICF element's records.  Synchronises `stream` once, as the block read does; not capture-safe.
 *   gf_block_read_downsampled_elems is the same for bytes, coarse blocks and statuses in host memory.
 * GF_ERR_ARG, before the context or a device is looked at: null pointers or a null entry of either pointer array, n_elems < 1 or
 * > GF_MAX_ELEMS, a type outside 0..3, factor < 1, block.n_rows < 1, block.n_cols < 1, row0 < 0 or col0 < 0, a SHORT fill_i outside
 * int16, a block or output pointer that is not 4-byte aligned, and for the record forms whatever gf_block_read_elems[_dev] rejects.
 * GF_ERR_UNSUPPORTED: factor > 46340 (f * f leaves Java's int: the reference's new int[nRows * nColumns] fails; the rectangle rule
 * answers the same), GF_ELEM_ICF in the two plain forms.                                                                         */
gf_status gf_block_downsample_rect(const gf_rect *block, int factor, gf_rect *out);
gf_status gf_block_downsample_elems_dev(gf_context *ctx, void *stream, const gf_elem_spec *elems, int n_elems, const gf_rect *block,
                                        int factor, const void *const *d_blocks, void *const *d_out);
gf_status gf_block_downsample_elems(gf_context *ctx, const gf_elem_spec *elems, int n_elems, const gf_rect *block, int factor,
                                    const void *const *blocks, void *const *out);
gf_status gf_block_read_downsampled_elems_dev(gf_context *ctx, void *stream, const int *codecs, int n_codecs, const gf_elem_spec *elems,
                                              int n_elems, const gf_grid_spec *grid, const gf_rect *rect, int factor, size_t n_records,
                                              const uint8_t *d_blob, size_t blob_bytes, const uint64_t *d_offsets, int verify_checksum,
                                              void *const *d_out, int32_t *d_status);
gf_status gf_block_read_downsampled_elems(gf_context *ctx, const int *codecs, int n_codecs, const gf_elem_spec *elems, int n_elems,
                                          const gf_grid_spec *grid, const gf_rect *rect, int factor, size_t n_records, const uint8_t *blob,
                                          const uint64_t *offsets, int verify_checksum, void *const *out, int32_t *status);

/* ---- a grid block TABULATED: value counts, range and entropy, in device memory ----------------------------------------------------
 * (demo/src/main/java/org/gridfour/demo/globalDEM/InputDataStatCollector.java:55-108, PackageData.java:445-448, :465-466, :504-533,
 * ExtractData.java:306-317; demo/src/main/java/org/gridfour/demo/entropy/EntropyTabulator.java:227-297, util/KahanSummation.java:63-69)
 * What the reference's data assessment says about a raster, over a block that lies in device memory: n_cells cells, row-major and
 * contiguous as gf_block_read_elems_dev delivers them -- int32 (INT), int16 (SHORT), float32 (FLOAT), the pointer 4-byte aligned.
 * GF_ELEM_ICF is refused with GF_ERR_UNSUPPORTED: read the element as INT codes, or tabulate the float block as FLOAT.  Everything
 * delivered is integers or the result of a comparison with a definite tie rule: bit-exact whatever the order of evaluation.
 *   DENSE FORM: InputDataStatCollector beside PackageData's zMin / zMax / zSum, quirks included.
 *   gf_tab_dense_plan_of (host arithmetic only), the constructor: n_counter = (int)((def_max - def_min + 1) * scale), the difference a
 *   Java int (it wraps), the product in double with the scale as given, the cast Java's (truncating, saturating, NaN -> 0); base =
 *   (int)(def_min * scale); n_bins = n_counter + 1 counters; scale_used = (double)(float) scale -- the constructor stores the scale
 *   through a float, so the plan and the samples see two different scales.  GF_ERR_ARG: n_counter < 0, a scale that is NaN or <= 0;
 *   GF_ERR_UNSUPPORTED: n_bins > 2^28.
 *   Per cell, the value taken as a double: a NaN is no sample, and under GF_TAB_SKIP_FILL an INT / SHORT cell equal to fill_i is none
 *   either (both count in n_skipped).  A sample: sample = (int)(v * scale_used + 0.5) in FP64 without fma, index = sample - base with
 *   int32 wrap; index < 0 or index > n_counter touches no counter and neither n_samples nor sum_samples, but still counts for min /
 *   max / sum_i; else counter[index]++, sum_samples += sample, n_samples++.  (The cast truncates toward zero: at scale 1 the int -3
 *   is sample -2.)  The reference's mean is sum_samples / n_samples / scale_used: the caller's arithmetic.
 *   min / max are zMin / zMax: they start at +-infinity and are replaced on a strict < / >, so each is the value of the FIRST cell in
 *   row-major order that compares equal to the extreme (which decides between +0.0 and -0.0), and min_at / max_at is first_cell +
 *   that cell's index (-1: no sample).  sum_i is the exact int64 sum of all samples of an INT / SHORT block (0 for FLOAT); it equals
 *   zSum wherever every partial sum stays below 2^53.  No float sum is offered: a sequential double sum of floats has an order.
 *   Without GF_TAB_ACCUMULATE the call itself initialises d_counter[0 .. n_bins) and *d_summary; with it the call adds to what is
 *   there -- a raster goes through in strips with first_cell as the reference's row loop does, and ties in min / max go to the smaller
 *   global index.  n_cells == 0 is GF_OK: it initialises unless accumulating and reads nothing; more than 2^40 cells in one call is
 *   GF_ERR_UNSUPPORTED (go through in strips).  The device form ONLY ENQUEUES on
 *   `stream` (NULL: the context's) and writes exactly n_bins counters and the summary; a small fixed-size scratch of the context is
 *   allocated on the first call.  gf_block_tabulate_dense is the same for block, counters and summary in host memory (accumulating, it
 *   uploads what they hold), staged through a buffer of the context; it synchronises.
 *   SYMBOL FORM: EntropyTabulator's count of every distinct 32-bit symbol -- an INT cell's bits, a SHORT cell sign-extended, a FLOAT
 *   cell's RAW bits (-0.0 and +0.0 are two symbols, every NaN payload its own); every cell counts, the fill included.  The table is
 *   what the reference's count file holds, compacted: the distinct symbols in ascending UNSIGNED order (negative ints behind the
 *   positive ones), each with its count.  n_samples = n_cells, n_symbols the distinct symbols, n_unique those with count 1, n_repeated
 *   the rest, max_count the largest count.  With n_symbols > table_cap the first table_cap entries are written, n_written = table_cap,
 *   the scalars are complete, and the host form returns GF_ERR_CAPACITY; table_cap == 0 with NULL tables asks for the scalars alone.
 *   n_cells > 2^31 - 1 in one call: GF_ERR_UNSUPPORTED (a count is a Java int); a larger raster goes through in strips with the
 *   accumulate form below.  The call grows a temporary of the context on demand (9 bytes per cell) and only enqueues; it is not
 *   claimed safe for hipGraph capture.  It always writes reserved = 0, and a SHORT block takes the same sort as the others.
 *   TABLES MERGED, STRIPS ACCUMULATED: a TABLE is what the symbol form writes -- n symbols in strictly ascending unsigned order, each
 *   with an int32 count, and a gf_tab_symbols summary; its entries that count are the first min(n_written, cap), which the device
 *   forms read on the device (the host passes upper bounds only, so they only enqueue and never synchronise).
 *   gf_tab_symbols_merge_dev: the union of the symbols of tables A and B in ascending unsigned order; the count of a symbol that both
 *   hold is the sum with INT32 WRAP, as the reference's counter, a Java int, wraps on count + 1 (EntropyTabulator.java:239-240) --
 *   addition mod 2^32 is associative, so any split of a raster into strips gives the counts of the one loop.  An entry whose count
 *   wrapped to <= 0 stays in the table (it records a symbol that was seen; gf_tab_entropy_counts skips it).  n_samples is the int64
 *   sum of the inputs', n_symbols the entries of the result, and n_unique, n_repeated and max_count are taken over the entries with
 *   count > 0 alone, as the reference's last loop does (:278-292; max_count is 0 where there is none).  THE ONE DEVIATION: the
 *   reference's nSymbols counts a symbol once more when its counter comes back to 0 after 2^32 occurrences; n_symbols here is the
 *   number of distinct symbols.  Capacity as above: with more entries than table_cap the first table_cap are written, n_written =
 *   table_cap, the scalars are complete, and the host form returns GF_ERR_CAPACITY.  An input that does not hold all of its symbols
 *   (fewer entries that count than its n_symbols) cannot give a complete result: the merge takes the entries it has and sets
 *   GF_TAB_SYM_INPUT_TRUNCATED (bit 0) in the result's reserved field; an input that carries the bit hands it on, and the host
 *   form returns GF_ERR_CAPACITY.  Inputs that are not strictly ascending give an unspecified table, but never a write outside
 *   [0, table_cap) or a read outside the inputs' entries.  The output arrays and summary must not overlap one another or any input
 *   (the caller keeps two tables and alternates); an input table of more than 2^31 - 1 entries is GF_ERR_UNSUPPORTED.
 *   gf_block_tabulate_symbols_acc_dev: the symbol form of one strip of n_cells <= 2^31 - 1 cells into a table of the context (INT,
 *   FLOAT: the sort above; SHORT: 65,536 counters, no widening and no sort), merged with the caller's in-table into the out table.
 *   The total over the calls is unbounded (n_samples is an int64).  No in-table -- NULL arrays, a NULL summary, cap_in == 0 -- or one
 *   whose summary has n_samples == 0 is empty; n_cells == 0 copies the in-table through.  GF_ELEM_ICF is refused as above.  A SHORT
 *   block need only be 2-byte aligned here, so strips with odd cell counts follow one another in one array.  Temporary of the
 *   context: 17 bytes per cell of the strip (SHORT: 768 KiB) and 8 bytes per 2,048 entries of the tables.
 *   gf_block_read_tabulated_symbols_elems[_dev]: gf_block_read_elems[_dev] of one rectangle into a temporary of the context, then
 *   the accumulate form for element `which`; a GF_ELEM_ICF element is taken as its INT codes, which is what the reference's
 *   readValueInt delivers for it (EntropyTabulator.java:230-235).  d_status as the block read defines it: the table is good iff
 *   every status is 0.
 *   gf_tab_symbols_merge, gf_block_tabulate_symbols_acc: the same for host memory, staged through a buffer of the context; an input
 *   goes up with the entries that count.  They synchronise.
 *   THESE DEVICE FORMS TAKE NO `void *stream`: like the gf_image_* and gf_lsop08_* calls they enqueue on the context's own stream.
 *   gf_tab_entropy_counts (host only): bits per sample from counts in the order given, counts <= 0 skipped.  kahan = 1 is
 *   EntropyTabulator's sum: p = count / (double) n_samples, s = -p * log(p), added with KahanSummation.add as written, the sum divided
 *   by log(2.0).  kahan = 0 is InputDataStatCollector.getEntropy: sum += p * log(p), -sum / log(2.0), and 0 for n_samples == 0.
 *   ORDER: every tabulation call of a context uses the same scratch of that context (the dense form's partials; the temporary of
 *   the symbol form, of the merge and of the accumulate form, which a later, larger call frees and replaces).  The calls themselves are serialised by the context's lock, but what
 *   they enqueue is not: tabulation calls on one context must all go to ONE stream, or the caller orders the streams (an event
 *   between them) so that no two are in flight at once.  Contexts are independent of one another.
 * GF_ERR_ARG, before the context or a device is looked at: a NULL ctx, block, spec, summary or counter array; NULL tables with
 * table_cap > 0; an element type outside 0..3; a SHORT fill_i outside int16; n_cells < 0 or first_cell < 0; a block, counter or table
 * pointer that is not 4-byte aligned, a summary pointer that is not 8-byte aligned; unknown flag bits; the plan's errors.  Then
 * GF_ERR_UNSUPPORTED as listed.  The merge and the accumulate form, in this order: a NULL ctx, block or summary (the merge: any of
 * the three; the accumulate form: the out summary); an element type outside 0..3, n_cells < 0; a block that is not 4-byte (SHORT:
 * 2-byte) aligned; an in-table with one array and not the other; an out table with table_cap > 0 and a NULL array, or misaligned;
 * an input table with cap > 0 and a NULL array (the merge), or misaligned; outputs that overlap one another or an input: all
 * GF_ERR_ARG.  Then GF_ERR_UNSUPPORTED: GF_ELEM_ICF, n_cells > 2^31 - 1, an input cap > 2^31 - 1.                                */
typedef struct gf_tab_dense { int32_t def_min, def_max; double scale; } gf_tab_dense;
typedef struct gf_tab_dense_plan { int32_t n_counter, base; int64_t n_bins; double scale_used; } gf_tab_dense_plan;
typedef struct gf_tab_summary {          /* device memory, 8-byte aligned */
    int64_t n_cells, n_skipped;          /* cells looked at; cells that are no sample (NaN; the fill under GF_TAB_SKIP_FILL) */
    int64_t n_samples, sum_samples;      /* the collector's nSamples and sumSamples (Java long, wraps)                       */
    int64_t sum_i;                       /* INT, SHORT: exact sum of all samples; FLOAT: 0                                   */
    double  min, max;                    /* zMin, zMax; +inf / -inf where there is no sample                                 */
    int64_t min_at, max_at;              /* first_cell + row-major index of the cell that holds them; -1: none              */
} gf_tab_summary;
#define GF_TAB_ACCUMULATE 1
#define GF_TAB_SKIP_FILL  2
typedef struct gf_tab_symbols { int64_t n_samples, n_symbols, n_unique, n_repeated, n_written; int32_t max_count, reserved; } gf_tab_symbols;
gf_status gf_tab_dense_plan_of(const gf_tab_dense *spec, gf_tab_dense_plan *plan);
gf_status gf_block_tabulate_dense_dev(gf_context *ctx, void *stream, int elem_type, int32_t fill_i, int flags, const void *d_block,
                                      int64_t n_cells, int64_t first_cell, const gf_tab_dense *spec, int32_t *d_counter,
                                      gf_tab_summary *d_summary);
gf_status gf_block_tabulate_dense(gf_context *ctx, int elem_type, int32_t fill_i, int flags, const void *block, int64_t n_cells,
                                  int64_t first_cell, const gf_tab_dense *spec, int32_t *counter, gf_tab_summary *summary);
gf_status gf_block_tabulate_symbols_dev(gf_context *ctx, void *stream, int elem_type, const void *d_block, int64_t n_cells,
                                        uint32_t *d_symbols, int32_t *d_counts, size_t table_cap, gf_tab_symbols *d_summary);
gf_status gf_block_tabulate_symbols(gf_context *ctx, int elem_type, const void *block, int64_t n_cells, uint32_t *symbols,
                                    int32_t *counts, size_t table_cap, gf_tab_symbols *summary);
#define GF_TAB_SYM_INPUT_TRUNCATED 1      /* gf_tab_symbols.reserved, bit 0: an input of a merge did not hold all of its symbols */
gf_status gf_tab_symbols_merge_dev(gf_context *ctx, const uint32_t *d_sym_a, const int32_t *d_cnt_a, const gf_tab_symbols *d_sum_a,
                                   size_t cap_a, const uint32_t *d_sym_b, const int32_t *d_cnt_b, const gf_tab_symbols *d_sum_b,
                                   size_t cap_b, uint32_t *d_sym_out, int32_t *d_cnt_out, size_t table_cap, gf_tab_symbols *d_sum_out);
gf_status gf_tab_symbols_merge(gf_context *ctx, const uint32_t *sym_a, const int32_t *cnt_a, const gf_tab_symbols *sum_a, size_t cap_a,
                               const uint32_t *sym_b, const int32_t *cnt_b, const gf_tab_symbols *sum_b, size_t cap_b,
                               uint32_t *sym_out, int32_t *cnt_out, size_t table_cap, gf_tab_symbols *sum_out);
gf_status gf_block_tabulate_symbols_acc_dev(gf_context *ctx, int elem_type, const void *d_block, int64_t n_cells,
                                            const uint32_t *d_sym_in, const int32_t *d_cnt_in, const gf_tab_symbols *d_sum_in,
                                            size_t cap_in, uint32_t *d_sym_out, int32_t *d_cnt_out, size_t cap_out,
                                            gf_tab_symbols *d_sum_out);
gf_status gf_block_tabulate_symbols_acc(gf_context *ctx, int elem_type, const void *block, int64_t n_cells, const uint32_t *sym_in,
                                        const int32_t *cnt_in, const gf_tab_symbols *sum_in, size_t cap_in, uint32_t *sym_out,
                                        int32_t *cnt_out, size_t cap_out, gf_tab_symbols *sum_out);
gf_status gf_block_read_tabulated_symbols_elems_dev(gf_context *ctx, const int *codecs, int n_codecs, const gf_elem_spec *elems, int n_elems,
                                                    const gf_grid_spec *grid, const gf_rect *rect, size_t n_records, const uint8_t *d_blob,
                                                    size_t blob_bytes, const uint64_t *d_offsets, int verify_checksum, int which,
                                                    const uint32_t *d_sym_in, const int32_t *d_cnt_in, const gf_tab_symbols *d_sum_in,
                                                    size_t cap_in, uint32_t *d_sym_out, int32_t *d_cnt_out, size_t cap_out,
                                                    gf_tab_symbols *d_sum_out, int32_t *d_status);
gf_status gf_block_read_tabulated_symbols_elems(gf_context *ctx, const int *codecs, int n_codecs, const gf_elem_spec *elems, int n_elems,
                                                const gf_grid_spec *grid, const gf_rect *rect, size_t n_records, const uint8_t *blob,
                                                const uint64_t *offsets, int verify_checksum, int which, const uint32_t *sym_in,
                                                const int32_t *cnt_in, const gf_tab_symbols *sum_in, size_t cap_in, uint32_t *sym_out,
                                                int32_t *cnt_out, size_t cap_out, gf_tab_symbols *sum_out, int32_t *status);
gf_status gf_tab_entropy_counts(const int32_t *counts, size_t n, int64_t n_samples, int kahan, double *entropy);

/* ---- a grid block WRITTEN: raster in, tile records out, in device memory ------------------------------------------------------
 * (gvrs/TileElementInt.java:118-126, TileElementShort.java:136-143, TileElementFloat.java:133-149, TileElementIntCodedFloat.java:152-169
 * setValue / setIntValue; TileElement*.hasValidData, gvrs/RasterTile.java:215-222; gvrs/RecordManager.java:386-490 writeTile, :413-419)
 * What the reference's tile cache and record manager produce when a rectangle of the raster is stored: the composition of the cut
 * (gf_tiles_from_block_dev), the tile cache's range checks and float-to-code conversion, its "has valid data" verdict, the merge
 * with what the file already holds, and gf_tile_record_encode_batch_elems_dev.
 *   gf_block_tile_rect: the rectangle of tiles a rect touches, first tile row / column and the counts (host arithmetic only).
 *   OUTPUT: one entry per tile of that rectangle of tiles, n_out = n_tile_rows * n_tile_cols, row-major.  d_tile_indices[j]: the
 *   tile's index on the grid.  Record j is d_blob[d_offsets[j] .. d_offsets[j+1]), n_out + 1 offsets, d_offsets[0] = 0; d_codec_used
 *   (may be NULL, element-major) and d_status[j] (per tile) as gf_tile_record_encode_batch_elems_dev defines them, the same capacity
 *   rule (a record that would end behind blob_cap is skipped whole), d_blob 8-byte aligned.  A tile that gets no record (a status
 *   other than GF_OK) has length 0 and 255 in its d_codec_used entries.
 *   INPUT: d_blocks (a HOST array of n_elems device pointers, each 4-byte aligned): the rectangle's cells, row-major, in the type a
 *   user writes: int32 (INT), int16 (SHORT), float32 (FLOAT) and float32 VALUES for ICF, not codes.  A cell whose grid coordinate
 *   lies in the rectangle takes the block's value; every other cell of a tile, those beyond the grid included, takes the element's
 *   fill: fill_i for INT and SHORT, the code fill_i for ICF, fill_f for FLOAT -- unless the tile has an old record, see below.
 *   ICF, per cell, as setValue: bits equal to fill_f's (any NaN matches a NaN fill, +0.0 and -0.0 differ: Float.equals) -> the code
 *   fill_i; else min_f <= v <= max_f -> (int) Math.floor((double)((v - offset) * scale) + 0.5), the subtraction and the product each
 *   rounded once in float32, the cast saturating as Java's; else out of range.
 *   RANGES (ranges[e]; NULL: the reference's default constructors): INT [INT_MIN + 1, INT_MAX] and SHORT [-32767, 32767]: a cell
 *   passes when it is in [min_i, max_i] or equals the fill; FLOAT [-inf, +inf]: in [min_f, max_f] or its bits equal the fill's as
 *   above (a NaN with a non-NaN fill is out of range); ICF min_f = (float)(INT_MIN + 1) / scale + offset, max_f = (float)(INT_MAX - 1)
 *   / scale + offset in float32 (min_i / max_i are not consulted).  Any out-of-range cell of any element gives the tile
 *   GF_ERR_BOUNDS and no record (the reference throws IllegalArgumentException).
 *   NO VALID DATA: a tile in which every element is all fill after the merge (INT, SHORT: v != fill; ICF: code != fill_i; FLOAT with
 *   a NaN fill: !isnan(v), with another fill the float comparison v != fill) gets GF_DECLINED and no record: writeTile writes
 *   nothing for it and frees its old record, which the caller learns from the status.
 *   OLD RECORDS (n_old may be 0, the three arguments then NULL): records the file already holds, in any order, decoded with
 *   gf_tile_record_decode_batch_elems_dev's pipeline (ICF elements as their codes) into a temporary of the context.  Of two records
 *   of one tile the later wins.  A partly covered tile with an old record keeps the old cells outside the rectangle; without one
 *   it is a new tile and takes fill there.  If the winning old record of a partly covered tile has an element whose status is not
 *   GF_OK, the tile gets that status (the first such element) and no record.  OLD RECORDS OF WHOLLY COVERED TILES, AND OF TILES
 *   OUTSIDE THE RECTANGLE, ARE DECODED AND IGNORED, as in the block read.
 *   LIMITATION: an old record whose HEADER cannot be read (its size field too small, too large or no multiple of 8, a record type
 *   other than a tile's) names no tile, as in the block read, and the old records' statuses are not returned: a partly covered
 *   tile whose only, or later, old record is damaged in this way is treated as a tile the file does not hold yet -- written with
 *   fill outside the rectangle, status GF_OK -- and the earlier of two records wins when the later one's header is damaged.  A
 *   caller that cannot trust its record headers decodes them first (gf_tile_record_decode_batch_elems_dev reports every record).
 *   A tile's status, first match: old-record failure, GF_ERR_BOUNDS, GF_DECLINED, the record writer's own verdict.
 * With n_old == 0 the device form ONLY ENQUEUES on `stream` and never synchronises; with old records it synchronises `stream` once,
 * as the decode does.  Graph capture is not claimed for either.  It grows buffers of the context on demand (cut tiles, flags, and
 * the block read's temporaries and slot table for the old records): a context's block reads, gathers and block writes belong on ONE
 * stream, or are ordered by the caller.
 * The device form takes the codec lists gf_tile_record_encode_batch_elems_dev takes (GF_ERR_UNSUPPORTED otherwise, from the arguments
 * alone).  GF_ERR_ARG, before the context or a device is looked at: whatever the block calls above reject of grid and rect,
 * whatever gf_tile_record_encode_batch_elems[_dev] rejects (n_rows, n_cols: the tile's; d_values: d_blocks) and, with n_old > 0,
 * gf_tile_record_decode_batch_elems[_dev]; a NULL d_status / status; a ranges[e] with min > max or a NaN float bound.
 * gf_block_write_elems is the same for host memory (no stream; old_offsets[n_old] bytes of old_blob are read) and takes any list:
 * it stages blocks and old records into buffers of the context and runs the same decode and cut; a list the device form accepts goes
 * through the device pipeline, any other list (one with CodecDeflate, as every standard list) brings the cut tiles and verdicts back
 * and sends the tiles that get a record through the host encoders of gf_tile_record_encode_batch_elems.  Every array is filled in;
 * it returns the first negative per-tile status as its own (GF_DECLINED is not an error), else GF_ERR_CAPACITY with
 * offsets[n_out] filled in when blob_cap is too small.                                                                          */
typedef struct gf_elem_range { int32_t min_i, max_i; float min_f, max_f; } gf_elem_range;
gf_status gf_block_tile_rect(const gf_grid_spec *grid, const gf_rect *rect, int32_t *tile_row0, int32_t *tile_col0,
                             int32_t *n_tile_rows, int32_t *n_tile_cols);
gf_status gf_block_write_elems_dev(gf_context *ctx, void *stream, const int *codecs, int n_codecs, const gf_elem_spec *elems,
                                   const gf_elem_range *ranges, int n_elems, const gf_grid_spec *grid, const gf_rect *rect,
                                   const void *const *d_blocks, size_t n_old, const uint8_t *d_old_blob, size_t old_blob_bytes,
                                   const uint64_t *d_old_offsets, int verify_old_checksum, int checksum_enabled, uint8_t *d_blob,
                                   size_t blob_cap, uint64_t *d_offsets, int32_t *d_tile_indices, uint8_t *d_codec_used,
                                   int32_t *d_status);
gf_status gf_block_write_elems(gf_context *ctx, const int *codecs, int n_codecs, const gf_elem_spec *elems,
                               const gf_elem_range *ranges, int n_elems, const gf_grid_spec *grid, const gf_rect *rect,
                               const void *const *blocks, size_t n_old, const uint8_t *old_blob, const uint64_t *old_offsets,
                               int verify_old_checksum, int checksum_enabled, uint8_t *blob, size_t blob_cap, uint64_t *offsets,
                               int32_t *tile_indices, uint8_t *codec_used, int32_t *status);

/* ---- ARGB IMAGES as element planes and as overviews, in device memory -----------------------------------------------------------
 * (demo/src/main/java/org/gridfour/demo/imaging/ExperimentalImageStorage.java:203-213 elements r, g, b; :242-256 elements Y, Co, Cg
 * after the reversible YCoCg-R transform; :275-286 the planes read back into words;
 * demo/src/main/java/org/gridfour/demo/geoTiff/DemoCOG.java:735-770 makeReducedImage)
 * What the reference does with an int[] argb, such as gf_block_render_* delivers: store it as three elements of a raster, read it
 * back, and compute its overview levels.  All arithmetic is Java's wrapping 32-bit int, bit for bit.
 *   SPLIT: r = (w >> 16) & 0xff, g = (w >> 8) & 0xff, b = w & 0xff; alpha is ignored.  GF_IMAGE_RGB: the planes are r, g, b.
 *   GF_IMAGE_YCOCG: Co = r - b; tmp = b + (Co >> 1); Cg = g - tmp; Y = tmp + (Cg >> 1); the planes are Y, Co, Cg.  Every plane value
 *   fits int16: elem_type GF_ELEM_INT writes int32 planes, GF_ELEM_SHORT int16 planes.
 *   JOIN, of ANY three ints (planes may hold fill or damaged values; an int16 is sign-extended as TileElementShort.getValueInt):
 *   YCoCg undoes the transform, tmp = Y - (Cg >> 1); g = Cg + tmp; b = tmp - (Co >> 1); r = b + Co; then both models give
 *   word = (((0xff00 | r) << 8 | g) << 8) | b, without masks: r = 256 gives a red byte of 0, r = -1 gives 0xffff0000 | g << 8 | b.
 *   The reference has no read loop of its own for r, g, b: the RGB join is its YCoCg loop without the transform.
 *   With every plane INT_MIN (a missing tile under fill_i = INT_MIN) both models give 0xff000000.  RGB: 0xff00 | r = 0x8000ff00,
 *   << 8 = 0x00ff0000, | g = 0x80ff0000, << 8 = 0xff000000, | b = 0xff000000.  YCoCg: Cg >> 1 = -2^30, tmp = -2^31 + 2^30 = -2^30,
 *   g = -2^31 - 2^30 = 2^30 (wrapped), b = -2^30 + 2^30 = 0, r = INT_MIN; 0x00ff0000 | 2^30 = 0x40ff0000, << 8 = 0xff000000, | 0.
 *   REDUCE by factor f: the reduced image has width / f x height / f words (gf_image_reduce_size, host arithmetic); word (i, j) is,
 *   over the f x f window at (i * f, j * f), n = f * f: the channels summed, c = (cSum + n / 2) / n, 0xff000000 | r << 16 | g << 8 | b.
 *   The rounding is not ExampleDownsample's: gf_block_downsample_* computes something else.  Rows and columns beyond the last whole
 *   window are not looked at.
 *   gf_image_split_dev / gf_image_join_dev: d_argb: n_pixels int32 in device memory, 4-byte aligned; d_planes: a HOST array of 3
 *   device pointers, each to n_pixels items, 4-byte (INT) or 2-byte (SHORT) aligned.  gf_image_reduce_dev: d_argb: height rows of
 *   width words, d_out: the reduced image, both 4-byte aligned.  Every output item is written exactly once; nothing outside the
 *   arrays is read or written.  These three ONLY ENQUEUE, allocate nothing, never synchronise, and are safe to capture on the
 *   context's stream.  gf_image_split / gf_image_join / gf_image_reduce are the same for host memory, staged through a buffer of the
 *   context, synchronising: a convenience, not a rate.
 *   gf_image_write_dev: rect's pixels (d_argb: rect.n_rows x rect.n_cols words, row-major) are split into three temporaries of the
 *   context, which grow on demand; then exactly the block write of gf_block_write_elems_dev runs with three elements of elem_type,
 *   fill fill_i and the type's whole range ([INT_MIN, INT_MAX], [-32768, 32767]: no cell is out of range).  Its outputs, statuses,
 *   capacity rule, d_tile_indices, d_codec_used and accepted codec lists are the block write's; so is its stream class: it only
 *   enqueues with n_old == 0 and synchronises once with old records.
 *   gf_image_read_dev: gf_block_read_elems_dev into three temporaries, then the join.  d_status is element-major, 3 * n_records
 *   entries, as the block read reports it.  The cells of absent or failed tiles are fill_i and go through the join like any other
 *   int.  Synchronises once, as the block read does.
 *   gf_image_write / gf_image_read: the same for host memory, as gf_block_write_elems / gf_block_read_elems stage; any codec list.
 * THESE CALLS TAKE NO STREAM ARGUMENT.  They run on the context's stream, which gf_context_stream hands out.  A caller orders other
 * work against that stream, or passes it (or NULL) to the other device forms of a chain.  The reason: tests/test_caller_stream_table.py
 * requires a row in tests/caller_stream.py for every function of this header whose declaration has a `void *stream` parameter, so a
 * stream parameter arrives in a later change.
 * Each of the following is checked before the context or a device is looked at:
 *   GF_ERR_ARG: a null pointer, or a null entry of a plane array;
 *   GF_ERR_ARG: a model outside 0 .. 1;
 *   GF_ERR_ARG: an elem_type other than GF_ELEM_INT / GF_ELEM_SHORT;
 *   GF_ERR_ARG: a SHORT fill_i outside int16 (the record forms);
 *   GF_ERR_ARG: a misaligned device pointer;
 *   GF_ERR_ARG: width, height or factor < 1;
 *   GF_ERR_UNSUPPORTED: factor > 2899 (2899^2 * 255 + 2899^2 / 2 = 2,147,273,355 still fits an int and 2900^2 does not: beyond it
 *   the reference's sums wrap);
 *   GF_ERR_UNSUPPORTED: more than 2^48 pixels;
 *   GF_OK, nothing written: n_pixels == 0; an empty reduced image (factor > width or factor > height);
 *   the record forms: whatever gf_block_write_elems[_dev] / gf_block_read_elems[_dev] reject, with the code they give.          */
#define GF_IMAGE_RGB 0
#define GF_IMAGE_YCOCG 1
gf_status gf_image_split_dev(gf_context *ctx, int model, int elem_type, size_t n_pixels, const int32_t *d_argb, void *const *d_planes);
gf_status gf_image_join_dev(gf_context *ctx, int model, int elem_type, size_t n_pixels, const void *const *d_planes, int32_t *d_argb);
gf_status gf_image_reduce_size(int width, int height, int factor, int *out_width, int *out_height);
gf_status gf_image_reduce_dev(gf_context *ctx, int width, int height, int factor, const int32_t *d_argb, int32_t *d_out);
gf_status gf_image_split(gf_context *ctx, int model, int elem_type, size_t n_pixels, const int32_t *argb, void *const *planes);
gf_status gf_image_join(gf_context *ctx, int model, int elem_type, size_t n_pixels, const void *const *planes, int32_t *argb);
gf_status gf_image_reduce(gf_context *ctx, int width, int height, int factor, const int32_t *argb, int32_t *out);
gf_status gf_image_write_dev(gf_context *ctx, const int *codecs, int n_codecs, int model, int elem_type, int32_t fill_i,
                             const gf_grid_spec *grid, const gf_rect *rect, const int32_t *d_argb, size_t n_old,
                             const uint8_t *d_old_blob, size_t old_blob_bytes, const uint64_t *d_old_offsets, int verify_old_checksum,
                             int checksum_enabled, uint8_t *d_blob, size_t blob_cap, uint64_t *d_offsets, int32_t *d_tile_indices,
                             uint8_t *d_codec_used, int32_t *d_status);
gf_status gf_image_read_dev(gf_context *ctx, const int *codecs, int n_codecs, int model, int elem_type, int32_t fill_i,
                            const gf_grid_spec *grid, const gf_rect *rect, size_t n_records, const uint8_t *d_blob, size_t blob_bytes,
                            const uint64_t *d_offsets, int verify_checksum, int32_t *d_argb, int32_t *d_status);
gf_status gf_image_write(gf_context *ctx, const int *codecs, int n_codecs, int model, int elem_type, int32_t fill_i,
                         const gf_grid_spec *grid, const gf_rect *rect, const int32_t *argb, size_t n_old, const uint8_t *old_blob,
                         const uint64_t *old_offsets, int verify_old_checksum, int checksum_enabled, uint8_t *blob, size_t blob_cap,
                         uint64_t *offsets, int32_t *tile_indices, uint8_t *codec_used, int32_t *status);
gf_status gf_image_read(gf_context *ctx, const int *codecs, int n_codecs, int model, int elem_type, int32_t fill_i,
                        const gf_grid_spec *grid, const gf_rect *rect, size_t n_records, const uint8_t *blob, const uint64_t *offsets,
                        int verify_checksum, int32_t *argb, int32_t *status);

/* ---- CodecFloat (compress/CodecFloat.java:328-458): float32 tiles ---------------------------
 * The five byte planes (sign bits, exponent, three byte-delta coded mantissa bytes) are split and
 * merged on the GPU; the Deflate stage of each plane runs on the host's zlib (its bytes are defined
 * by zlib itself: the reference calls java.util.zip.Deflater(9), CodecFloat.java:268-283).
 * plane buffer of a tile: [sign ceil(n/8)] [exponent n] [m1 n] [m2 n] [m3 n], n = n_rows*n_cols.   */
size_t gf_float_planes_bytes(int n_rows, int n_cols);
gf_status gf_float_planes_encode_dev(gf_context *ctx, void *stream, int n_rows, int n_cols, size_t n_tiles,
                                     const float *d_values, uint8_t *d_planes, size_t plane_stride);
gf_status gf_float_planes_decode_dev(gf_context *ctx, void *stream, int n_rows, int n_cols, size_t n_tiles,
                                     const uint8_t *d_planes, size_t plane_stride, float *d_values);
/* replaces ICompressionEncoder.encodeFloats / ICompressionDecoder.decodeFloats as implemented by
 * CodecFloat, for one tile or a batch in host memory.  zlib_level: 9 = current reference source,
 * 6 = what the reference's sample files were written with.  offsets[n_tiles+1] as for the int path. */
gf_status gf_float_encode_batch_f32(gf_context *ctx, int codec_index, int n_rows, int n_cols, size_t n_tiles,
                                    const float *values, int zlib_level, uint8_t *blob, size_t blob_cap,
                                    uint64_t *offsets);
gf_status gf_float_decode_batch_f32(gf_context *ctx, int n_rows, int n_cols, size_t n_tiles, const uint8_t *blob,
                                    const uint64_t *offsets, float *values, int32_t *status);
gf_status gf_float_encode_f32(gf_context *ctx, int codec_index, int n_rows, int n_cols, const float *values,
                              int zlib_level, uint8_t *out, size_t out_cap, size_t *out_len);
gf_status gf_float_decode_f32(gf_context *ctx, int n_rows, int n_cols, const uint8_t *packing, size_t packing_len,
                              float *values);

/* ---- synthetic elevation tiles (bench / tests) ---- */
/* fills n_tiles tiles of a seeded integer value-noise DEM cut into
 * n_rows x n_cols tiles, tiles_per_row tiles across, starting at tile0.      */
gf_status gf_synth_dem_dev(gf_context *ctx, void *stream, uint64_t seed, int n_rows, int n_cols,
                           int64_t tiles_per_row, int64_t tile0, size_t n_tiles,
                           int32_t *d_values);
/* the nulls workload of SURVEY.md section 8d: the same grid with an "ocean mask" -- mask_per_mille / 1000 of its
 * 16 x 16 blocks hold GF_INT4_NULL_CODE, so that nearly every tile takes PredictorModelDifferencingWithNulls
 * (compress/CodecHuffman.java:73-98, PredictorModelDifferencingWithNulls.java:66-166)                            */
gf_status gf_synth_dem_masked_dev(gf_context *ctx, void *stream, uint64_t seed, int n_rows, int n_cols,
                                  int64_t tiles_per_row, int64_t tile0, size_t n_tiles, int mask_per_mille,
                                  int32_t *d_values);
/* the same grid as another kind of surface.  GF_DEM_STYLE_ROUGH: provinces of mountains / plains / stripes so that each of
 * PredictorModelDifferencing / Linear / Triangle wins a share of the tiles (compress/CodecHuffman.java:100-110), and cliff and
 * scree blocks whose residuals need two and three M32 bytes (compress/CodecM32.java:270-311) -- the data SURVEY.md section 8d
 * describes ("mostly within +-126 with a tail into 2-3 byte codes"); GF_DEM_STYLE_CLASSIC is gf_synth_dem_masked_dev.        */
#define GF_DEM_STYLE_CLASSIC 0
#define GF_DEM_STYLE_ROUGH 1
gf_status gf_synth_dem_style_dev(gf_context *ctx, void *stream, uint64_t seed, int n_rows, int n_cols,
                                 int64_t tiles_per_row, int64_t tile0, size_t n_tiles, int mask_per_mille, int style,
                                 int32_t *d_values);

/* ---- GVRS files: the header record, the tile directory and block reads from a file image ------------------------------------
 * (gvrs/GvrsFile.java:341-483 the constructor GvrsFile(File, "r"), gvrs/GvrsFileSpecification.java:856-1052, 1154-1160,
 * gvrs/RecordManager.java:835-856 readTileDirectory, gvrs/TileDirectory.java:200-257, gvrs/TileDirectoryExtended.java,
 * gvrs/GvrsElement.java:298-404 readBlock)
 * A file IMAGE is the bytes of a .gvrs file, as read or mapped.  gf_file_open parses the header record -- the specification of
 * grid, tiles, elements and codec list -- and the 24-byte prefix of the tile directory; the block reads then need nothing from
 * the caller but the image and a rectangle.  Version 1.04 files; everything little-endian.
 *   gf_file_open needs no device and no context (host arithmetic on bytes, not a compute entry point).  It reads only the header
 *   record and the directory's prefix and never a byte at or behind image_bytes.  The handle keeps copies and holds no pointer into
 *   the image: the image may be an mmap and may go away after the call.  GF_ERR_FORMAT: a wrong magic, a version the reference
 *   rejects, a number of levels other than 1, a non-zero opened-for-writing time, an element type code outside 0..3, a header
 *   checksum mismatch where the specification enables checksums (and a non-zero checksum word where it does not: the writer leaves
 *   0 there, and a damaged flag byte must not switch the check off), a header record too small for its fields or a field that runs
 *   past the header record, tile or grid sizes < 1, a tile-directory position that is 0, not a multiple of 8 or in front of the
 *   content, a directory prefix that does not fit the image, a directory rectangle with a negative number or more entries than the
 *   grid has tiles.  GF_ERR_BOUNDS: anything of the header record that would be read at or behind image_bytes (a truncated
 *   image).  GF_ERR_UNSUPPORTED: versions 1.02 and 1.03 (another file head), more than GF_MAX_ELEMS elements or 255 codecs, 2^28 or more cells in a tile, more than 0x7fffffff tiles.  GF_ERR_ARG: null
 *   pointers.  gf_file_info: element types are GF_ELEM_*; an ICF element's fill_i is its iFill, fill_f its fFill, scale and offset
 *   the file's; SHORT and INTEGER take fill_i from their fill, FLOAT takes fill_f.  codecs[k] is the GF_CODEC_* kind of the k-th
 *   codec id ("GvrsHuffman", "GvrsDeflate", "GvrsFloat" -> GF_CODEC_NONE, "GvrsCanonicalHuffman", "LSOP12", "LSOP08") or
 *   GF_CODEC_UNKNOWN for an id the library has no decoder for: such a file opens, and its reads answer GF_ERR_UNSUPPORTED.
 *   gf_file_elem_name / gf_file_codec_id: the strings of the specification (owned by the handle; NULL for a bad number).
 *   gf_file_tile_position: the directory looked up in an image in HOST memory: *pos = the file position of the tile's record
 *   content (the tile-index word; the record's size word is 8 bytes in front of it), 0 for a tile the file does not hold.  The
 *   entry and the record head are judged as the device form judges them (below): GF_ERR_BOUNDS / GF_ERR_FORMAT, *pos = the entry's
 *   position.  GF_ERR_ARG: a tile index outside the grid's tiles.
 *   gf_file_read_block_elems_dev: GvrsElement.readBlock for every element of the file, the image in DEVICE memory.  d_image is
 *   8-byte aligned and readable to the end of the aligned 16-byte piece that holds its last byte.  T = the tiles of the rectangle's
 *   rectangle of tiles (gf_block_tile_rect), row-major; d_status is element-major, d_status[e * T + j]; d_present[j] (may be NULL)
 *   is 1 where the directory names a record for tile j (a non-zero entry, whatever becomes of it).  A tile the directory does not
 *   name -- an entry of 0, or a tile outside the directory's rectangle -- is GF_OK for every element and its cells are fill, as the
 *   reference delivers them.  k_file_locate reads the directory in place in d_image (compact entries: unsigned int32 * 8; extended:
 *   int64) and judges a position before it touches it: position >= content_pos + 8, a multiple of 8, position + 12 <= image_bytes,
 *   and the entry itself inside the image -- else GF_ERR_BOUNDS and nothing of the tile is read; the record's tile-index word must
 *   equal the slot's tile index, else GF_ERR_FORMAT (the check the reference left as a commented assertion,
 *   RecordManager.java:746-748).  The record [position - 8, min(image_bytes, position - 8 + size)) then goes through the pipeline
 *   of gf_block_read_elems_dev unchanged: framing, CRC-32C when verify_checksum (and the file's specification enables checksums: the
 *   records of a file without them carry a 0 there, and the reference does not look), partition by codec, the decoders, scatter, gather.
 *   Statuses, fill for failed elements and THE BLOCK IS GOOD IFF EVERY STATUS IS GF_OK are exactly as there.  Runs on the context's
 *   stream (as the gf_lsop08_*_dev and gf_image_*_dev calls do) and synchronises it once, not capture-safe; d_blocks is a HOST array of n_elems device pointers.  GF_ERR_UNSUPPORTED: a codec list that holds
 *   GF_CODEC_UNKNOWN.  GF_ERR_ARG: null pointers, an unaligned d_image, image_bytes < content_pos, a rectangle not wholly inside
 *   the grid.
 *   gf_file_read_block_elems: the same for an image, blocks, statuses and present flags in HOST memory: the rectangle's tiles are
 *   looked up in the host image and only their records are staged, end to end, into the context's staging buffer -- never the
 *   whole image -- and go through the contiguous path of gf_block_read_elems.
 * Not here: versions <= 1.03, the contents of the metadata directory (its position is reported; writing a new file and updating
 * one: below), the tile cache.                                                                                                */
#define GF_CODEC_UNKNOWN (-1)   /* an id the library has no decoder for: reported, never accepted by a call */
typedef struct gf_file gf_file;
typedef struct gf_file_info {
    int32_t version, subversion, checksum_enabled, raster_space, coordinate_system;
    gf_grid_spec grid;
    int32_t n_elems;  gf_elem_spec elems[GF_MAX_ELEMS];   /* GF_ELEM_* types; fill_i / fill_f / scale / offset from the file */
    int32_t n_codecs; int32_t codecs[255];                /* GF_CODEC_* kinds in list order, GF_CODEC_UNKNOWN where unmapped */
    uint64_t content_pos, tile_dir_pos, metadata_dir_pos, freespace_dir_pos;
    int32_t dir_extended, dir_row0, dir_col0, dir_n_rows, dir_n_cols;  uint64_t dir_entries_pos;
    double x0, y0, x1, y1, cell_size_x, cell_size_y, m2r[6], r2m[6];
} gf_file_info;
gf_status gf_file_open(const uint8_t *image, size_t image_bytes, gf_file **out);   /* host bytes; no device, no context */
void      gf_file_close(gf_file *f);
gf_status gf_file_get_info(const gf_file *f, gf_file_info *info);
const char *gf_file_elem_name(const gf_file *f, int e);
const char *gf_file_codec_id(const gf_file *f, int k);
const char *gf_file_product_label(const gf_file *f);
gf_status gf_file_tile_position(const gf_file *f, const uint8_t *image, size_t image_bytes, int32_t tile_index, uint64_t *pos);
gf_status gf_file_read_block_elems_dev(gf_context *ctx, const gf_file *f, const uint8_t *d_image, size_t image_bytes,
                                       const gf_rect *rect, int verify_checksum, void *const *d_blocks, int32_t *d_status,
                                       uint8_t *d_present);
gf_status gf_file_read_block_elems(gf_context *ctx, const gf_file *f, const uint8_t *image, size_t image_bytes,
                                   const gf_rect *rect, int verify_checksum, void *const *blocks, int32_t *status, uint8_t *present);

/* ---- GVRS files read at POINTS: cells and B-spline interpolation at scattered points, straight from a file image -----------------
 * (gvrs/GvrsElement.java readValue / readValueInt, gvrs/TileAccessIndices.java:78-92 computeAccessIndices,
 * gvrs/GvrsInterpolatorBSpline.java:283-334 z / zNormal, :374-484 the window)
 * The reference's primary read interface is one cell or one query point at a time, and its tile cache loads only the tiles a
 * point needs.  These calls do the same for a BATCH: they find the tiles the points touch, decode those tiles alone into a pool
 * of the context and sample the pool; no block is built.  A track across an ETOPO1-shaped grid decodes its few hundred tiles,
 * not the 12,960 of its bounding rectangle.
 *   gf_file_cells_tiles / gf_file_interp_tiles need no device and no context (host arithmetic, like gf_file_open): the distinct
 *   tiles the points touch, in ascending tile index.  *n_tiles is always the full count; at most tiles_cap entries are written;
 *   tiles may be NULL with a cap of 0, which is the way to size max_tiles.  A cell's tile is (row / n_rows_tile) * tiles across +
 *   col / n_cols_tile; a cell outside the grid touches none.  An interpolation point touches the tiles of its 4 x 4 window -- rows
 *   row0 .. row0 + 3, columns col0 .. col0 + n1 - 1 and, where the window wraps, columns 0 .. 3 - n1 -- and none when it has no
 *   window: a NaN coordinate, a point outside the fringe, a wrapped window the reference's readBlock rejects.
 *   THE DEVICE FORMS take the image in device memory as gf_file_read_block_elems_dev does (8-byte aligned, readable to the end of
 *   the aligned 16-byte piece that holds its last byte), coordinates and outputs in device memory, and run on the CONTEXT'S
 *   stream: they take no stream argument.  They synchronise that stream TWICE -- once to learn how many tiles are touched, once
 *   inside the records' pipeline -- and are not capture-safe; the sampling kernel is enqueued behind the second and not waited for.
 *   CELL READS (gf_file_read_points_elems_dev; d_values a HOST array of n_elems device pointers, d_values[e] of n_points items in
 *   the element's delivered type; d_status[e * n_points + i]): d_values[e][i] is bit for bit the cell gf_file_read_block_elems_dev
 *   delivers at (rows[i], cols[i]) for element e, the fill where the directory names no record for the tile.  A point outside the
 *   grid: GF_ERR_ARG for every element, the fill, and no tile touched (the reference throws).  Where the tile's directory entry or
 *   record is refused, or the element fails to decode, the point carries the status the block read puts at that tile and element,
 *   and the fill.  Duplicate points are fine; outputs are in point order.
 *   INTERPOLATION (gf_file_interp_points_dev; element elem of the file): of spec the fields wrap, target, the spacings and the
 *   fringes are read; n_rows_grid, n_cols_grid, block, elem_type and fill_i are NOT: they come from the file -- its grid, the whole
 *   grid as the block, element elem.  For every point outputs and status equal what gf_block_interp_points_dev gives over the
 *   whole-grid block of element elem read by gf_file_read_block_elems_dev: GF_ERR_ARG / GF_DECLINED / GF_OK in its order
 *   (GF_ERR_BOUNDS cannot arise).  ONE ADDITION: if element elem of any tile of the window did not decode to GF_OK, the point takes
 *   the status of the lowest-indexed such tile and all its outputs are NaN -- the block route silently interpolates fill there.
 *   max_tiles: the pool holds touched * cells items per element (in the buffer of the context the block reads decode into: one
 *   call at a time, one stream).  If the points touch more than max_tiles tiles the call returns GF_ERR_CAPACITY,
 *   *n_tiles_touched holds the count and NO output item and no status has been written.  Otherwise it returns GF_OK whatever the
 *   per-point statuses are and *n_tiles_touched is the count.  n_points == 0: GF_OK, a count of 0, nothing written; max_tiles == 0
 *   with points that touch nothing is GF_OK.  Checksums are verified only where the file enables them, as in the block read.
 *   THE HOST FORMS (gf_file_read_points_elems, gf_file_interp_points): image, coordinates and outputs in host memory.  The touched
 *   tiles come from the two host functions, their records are looked up in the host image and staged end to end -- never the whole
 *   image -- exactly as gf_file_read_block_elems stages; then the same device tail runs.
 * GF_ERR_ARG, before the context or a device is looked at: null pointers (coordinates may be NULL with n_points == 0; out->z is
 * required, the other outputs are not); an unaligned d_image; image_bytes < content_pos; elem out of range; wrap or target out of
 * range; with target >= GF_INTERP_FIRST a zero row_spacing, or a zero col_spacing without per-point spacings; normal with target
 * GF_INTERP_VALUE; a grid under 4 x 4 for the interpolation forms.  GF_ERR_UNSUPPORTED: a codec list that holds GF_CODEC_UNKNOWN;
 * more than 2^27 tiles in the grid (bitmap and prefixes stay under 16 MB each); n_points or max_tiles * n_elems beyond 0x7fffffff
 * (they travel as 32 bits in the pipeline).                                                                                       */
gf_status gf_file_cells_tiles(const gf_file *f, size_t n_points, const int32_t *rows, const int32_t *cols,
                              int32_t *tiles, size_t tiles_cap, size_t *n_tiles);
gf_status gf_file_interp_tiles(const gf_file *f, const gf_interp_spec *spec, size_t n_points, const double *rows,
                               const double *cols, int32_t *tiles, size_t tiles_cap, size_t *n_tiles);
gf_status gf_file_read_points_elems_dev(gf_context *ctx, const gf_file *f, const uint8_t *d_image, size_t image_bytes,
                                        size_t n_points, const int32_t *d_rows, const int32_t *d_cols, int verify_checksum,
                                        size_t max_tiles, void *const *d_values /* HOST array of n_elems device pointers */,
                                        int32_t *d_status /* [e * n_points + i] */, size_t *n_tiles_touched);
gf_status gf_file_read_points_elems(gf_context *ctx, const gf_file *f, const uint8_t *image, size_t image_bytes,
                                    size_t n_points, const int32_t *rows, const int32_t *cols, int verify_checksum,
                                    size_t max_tiles, void *const *values, int32_t *status, size_t *n_tiles_touched);
gf_status gf_file_interp_points_dev(gf_context *ctx, const gf_file *f, const uint8_t *d_image, size_t image_bytes, int elem,
                                    const gf_interp_spec *spec, size_t n_points, const double *d_rows, const double *d_cols,
                                    const double *d_col_spacing, int verify_checksum, size_t max_tiles,
                                    const gf_interp_out *out, size_t *n_tiles_touched);
gf_status gf_file_interp_points(gf_context *ctx, const gf_file *f, const uint8_t *image, size_t image_bytes, int elem,
                                const gf_interp_spec *spec, size_t n_points, const double *rows, const double *cols,
                                const double *col_spacing, int verify_checksum, size_t max_tiles,
                                const gf_interp_out *out, size_t *n_tiles_touched);

/* ---- GVRS files queried at COORDINATES: longitude / latitude or model x / y instead of rows and columns ---------------------------
 * (gvrs/GvrsInterpolatorBSpline.java:166-181 z, :222-248 zNormal, :120-131 du and dv; gvrs/GvrsFileSpecification.java:2122-2126
 * mapModelToGridPoint, :2159-2173 mapGeographicToGridPoint, :2198-2212 makeGridPointUsingFringe, :2230-2234 mapGridToGeoPoint,
 * :2101-2105 mapGridToModelPoint, :695-707 checkGeographicCoverage, :435-440 the fringes; util/Angle.java:57-85)
 * The rules are stated once (gvrs_coords.h), in double, in the reference's operation order, without fused multiply-add; Java's % is
 * fmod; toRadians(a) = a * 0.017453292519943295 (JDK 9 and later; JDK 8's a / 180.0 * PI differs in the last bit).
 *   TWO DELIBERATE DEVIATIONS.  (1) The cosine of the column-spacing rule is StrictMath.cos's value (fdlibm's algorithm, which is
 *   specified exactly); the reference calls Math.cos, which is specified to within 1 ulp and may return exactly that value: on a JVM
 *   where it does not, the spacing differs by that ulp for some latitudes.  A caller who needs another cosine passes per-point
 *   spacings.  (2) z() refuses |y| > 90.0001 by throwing (:169-172), zNormal() omits the check; here a point of a GEOGRAPHIC file
 *   (coordinate_system == 2) whose latitude has |lat| > 90.0001 is refused with the per-point status GF_ERR_ARG at every target
 *   (a NaN passes, as in Java, and is refused later by the window).  That keeps the cosine's argument below 3 pi / 4.
 *   THE COLUMN-SPACING RULE (:226-232, :291-299): geographic file: dx = cos(toRadians(lat)) * du, and dx < 1 -> 1; any other
 *   file: du.  lat is the query's y, or mapGridToGeoPoint's latitude for a point given in grid coordinates.
 *   gf_file_interp_spec fills EVERY field of spec from the file, as the reference's interpolator sets itself up: the grid, the whole
 *   grid as the block, element elem's type and fill_i, wrap (checkGeographicCoverage; 0 for a file that is not geographic),
 *   row_spacing = dv and col_spacing = du (rEarth * toRadians(cell size), rEarth = 6371007.2, for a geographic file; the cell
 *   sizes otherwise) and the four fringes (-0.5 - 4 ulp((double) n), n - 0.5 + 4 ulp((double) n)).
 *   gf_file_map_points, kind GF_MAP_GEO_TO_GRID / GF_MAP_MODEL_TO_GRID: (a, b) = (x, y) -- X IS THE LONGITUDE, Y THE LATITUDE, the
 *   argument order of z() -- to out_a = row, out_b = column, the GridPoint's integer row and column (irow, icol: floor(v + 0.5)
 *   with Java's saturating cast, snapped to 0 / n - 1 inside the fringe), the column spacing of the rule with the file's du, and
 *   status: GF_ERR_ARG where the latitude check refuses y (then NaN, NaN, 0, 0, NaN), else GF_OK.  Kind GF_MAP_GRID_TO_GEO /
 *   GF_MAP_GRID_TO_MODEL: (a, b) = (row, column) to out_a = x (the longitude), out_b = y (the latitude); irow, icol, col_spacing
 *   and status must be NULL.  Any output may be NULL except out_a and out_b.  The geo kinds work on any file (the reference's
 *   mapping functions do not ask which system is set); the latitude check and the spacing rule ask the file, as the interpolator does.
 *   gf_file_map_points_dev: the same for arrays in device memory, bit for bit; it ONLY ENQUEUES on the context's stream, allocates
 *   nothing, never synchronises and is safe for hipGraph capture.
 *   CELLS AT COORDINATES need no call of their own: GvrsElement.readValue(GridPoint) reads the GridPoint's integers, so irow / icol
 *   go to gf_file_read_points_elems[_dev].
 *   gf_file_interp_coords_tiles is gf_file_interp_tiles with the mapping in front; a refused point touches no tile.
 *   gf_file_interp_coords_dev is gf_file_interp_points_dev for points given as kind says -- GF_COORDS_GRID: (a, b) = (row, column),
 *   zInterpGrid / zNormalGrid; GF_COORDS_FILE: (a, b) = (x, y) as z() / zNormal() read them -- mapped in registers by the kernels
 *   that mark the tiles and sample the pool: no row, column or spacing array is written in between.  spec is read as there
 *   (target, the spacings, wrap and the fringes; the rest comes from the file); the normal case is a spec of gf_file_interp_spec.
 *   d_col_spacing NULL: the rule above with du = spec->col_spacing; not NULL: the caller's spacings, the rule is bypassed.
 *   d_col_spacing_used (may be NULL) receives the spacing each point was evaluated with and NaN for a point the latitude check
 *   refused; it always has a source -- the caller's array or the rule -- so no argument error belongs to it.  PER-POINT STATUS:
 *   first GF_ERR_ARG with NaN outputs for a point the latitude check refuses (it touches no tile); then the order of
 *   gf_file_interp_points_dev, its ONE ADDITION included.  Streams, the two synchronisations, max_tiles, GF_ERR_CAPACITY with
 *   nothing written and *n_tiles_touched are as there.  gf_file_interp_coords: the same through host memory, built as
 *   gf_file_interp_points is (the touched tiles come from gf_file_interp_coords_tiles' arithmetic; only their records are staged).
 * GF_ERR_ARG, before the context or a device is looked at: null pointers with the allowances of the section above (coordinates
 * may be NULL with n == 0); a kind out of range; a non-NULL irow, icol, col_spacing or status with a from-grid kind; what
 * gf_file_interp_points_dev refuses of spec, elem, out and the image; for gf_file_interp_spec a bad elem or target or a grid under
 * 4 x 4.  A NULL ctx is judged LAST: GF_ERR_NO_DEVICE on a machine without a HIP device (no context can be had there),
 * GF_ERR_ARG otherwise.                                                                                                          */
#define GF_COORDS_GRID 0   /* (row, col) as given: zInterpGrid / zNormalGrid                                  */
#define GF_COORDS_FILE 1   /* (x, y) as z() / zNormal() read them: longitude, latitude for a geographic file, */
                           /* model x, y through m2r otherwise                                                */
#define GF_MAP_GEO_TO_GRID 0
#define GF_MAP_MODEL_TO_GRID 1
#define GF_MAP_GRID_TO_GEO 2
#define GF_MAP_GRID_TO_MODEL 3
gf_status gf_file_interp_spec(const gf_file *f, int elem, int target, gf_interp_spec *spec);
gf_status gf_file_map_points(const gf_file *f, int kind, size_t n, const double *a, const double *b, double *out_a, double *out_b,
                             int32_t *irow, int32_t *icol, double *col_spacing, int32_t *status);
gf_status gf_file_map_points_dev(gf_context *ctx, const gf_file *f, int kind, size_t n, const double *d_a, const double *d_b,
                                 double *d_out_a, double *d_out_b, int32_t *d_irow, int32_t *d_icol, double *d_col_spacing,
                                 int32_t *d_status);
gf_status gf_file_interp_coords_tiles(const gf_file *f, int kind, const gf_interp_spec *spec, size_t n, const double *a,
                                      const double *b, int32_t *tiles, size_t tiles_cap, size_t *n_tiles);
gf_status gf_file_interp_coords_dev(gf_context *ctx, const gf_file *f, const uint8_t *d_image, size_t image_bytes, int elem, int kind,
                                    const gf_interp_spec *spec, size_t n_points, const double *d_a, const double *d_b,
                                    const double *d_col_spacing, int verify_checksum, size_t max_tiles, const gf_interp_out *out,
                                    double *d_col_spacing_used, size_t *n_tiles_touched);
gf_status gf_file_interp_coords(gf_context *ctx, const gf_file *f, const uint8_t *image, size_t image_bytes, int elem, int kind,
                                const gf_interp_spec *spec, size_t n_points, const double *a, const double *b,
                                const double *col_spacing, int verify_checksum, size_t max_tiles, const gf_interp_out *out,
                                double *col_spacing_used, size_t *n_tiles_touched);

/* ---- GVRS files WRITTEN: a new file image from a rectangle of the raster, in one call ------------------------------------------
 * (gvrs/GvrsFile.java:239-300 the constructor that writes the header, :584-616 close; gvrs/GvrsFileSpecification.java:1170-1285
 * write; gvrs/GvrsMetadata.java:217-234 write; gvrs/RecordManager.java:161-204, 218-219 a record's frame and size, :670-719
 * writeMetadata, :864-883 writeTileDirectory, :991-1017 writeMetadataDirectory, :87, 451-454 the extended directory;
 * gvrs/TileDirectory.java:266-290, gvrs/TileDirectoryExtended.java writeTilePositions / getStorageSize)
 * The inverse of gf_file_open and the file reads: the image of a NEW version 1.04 file, laid out as every finished file of the
 * reference is,
 *     file head | header record | metadata records | tile records | metadata directory | tile directory
 * with no free-space directory (its header word is 0).  Every record: [int32 size, a multiple of 8][type 0 0 0][content][zeros]
 * [CRC-32C of all bytes in front of it, or 0 in a file without checksums], size = multipleOf8(content + 12).  Given the facts a
 * reference file was written from, its metadata records' fields and its tile records in file order, gf_file_assemble returns the
 * reference's file byte for byte.
 *   THE FACTS (gf_file_facts; strings are 0-terminated bytes, NULL reads as "", at most 65535 bytes each): grid and tile sizes; per
 *   element its gf_elem_spec (type, fill_i / fill_f, scale, offset) and a gf_file_elem_facts: name, label, description, unit, the
 *   continuous flag and the range the header states -- has_range 0: the defaults of the reference's constructors, as ranges ==
 *   NULL in gf_block_write_elems (an ICF's min_i / max_i are then INT_MIN + 1 / INT_MAX - 1 and its min_f / max_f their values);
 *   INT and SHORT state min_i / max_i, FLOAT min_f / max_f, ICF all four.  THE RANGE OF AN ELEMENT IS ALSO WHAT THE FILE WRITES
 *   CHECK CELLS AGAINST.  elem_facts == NULL: elements named "e0", "e1", ... with defaults.  codec_ids: the strings of the
 *   specification's codec list; the kinds follow from them as gf_file_open maps them ("GvrsFloat" -> GF_CODEC_NONE), an id that
 *   maps to nothing is GF_ERR_UNSUPPORTED.  checksum_enabled, raster_space, coordinate_system, the six bounds and cell sizes,
 *   m2r[6] and r2m[6] are written as given (nothing is computed from coordinates); product label, UUID (the 16 bytes in file
 *   order), time modified.  Opened-for-writing is 0 and the number of levels 1.  The header record's size is the reference's:
 *   multipleOf8 of its fields + 8 reserved bytes + the checksum word.
 *   METADATA (gf_file_metadata, n_metadata of them, may be 0): name, record id, type code (GvrsMetadataType), content bytes and
 *   description; record content [utf name][int32 id][type 0 0 0][int32 n][n bytes][utf description], record type 1, laid in the
 *   caller's order directly behind the header record.  The metadata directory (record type 4: int32 count, then per record int64
 *   content position, utf name, int32 id, type byte, in order of position) follows the tile records; with n_metadata == 0 there is
 *   none and the header's word is 0.
 *   THE TILE DIRECTORY (record type 5): 8 prefix bytes (byte 1: the extended flag), int32 row0 col0 nRows nCols, the entries
 *   row-major.  The rectangle is the BOUNDING rectangle of the tiles that got a record; a tile inside it without one has entry 0.
 *   With no record at all the four numbers are 0, there are no entries and the record is 40 bytes.  Compact entries: content
 *   position / 8 as uint32; extended: int64 positions.  Extended when a record's content position exceeds 1 << 35, as the
 *   reference decides, or when flags holds GF_FILE_DIR_EXTENDED (any size; the readers take either form at any size).
 *   gf_file_write_plan (host arithmetic): *first_record_pos = where the first tile record goes (behind the metadata records, a
 *   multiple of 8); *max_image_bytes = the largest image the rectangle of tiles rect touches (NULL: the whole grid) can need: every
 *   tile's record at gf_tile_record_max_bytes_elems plus both directories.  Either pointer may be NULL.
 *   gf_file_assemble needs no device and no context.  Records as gf_tile_record_encode_batch_elems and gf_block_write_elems hand
 *   them out: record r = blob[offsets[r] .. offsets[r + 1]) belongs to tile tile_indices[r].  The image holds them IN THE CALLER'S
 *   ORDER (the reference's sample files lay their tiles 3, 2, 1, 0); a record of length 0 gets no place and its tile the entry 0.
 *   *image_bytes = the image's size, also when it does not fit: GF_ERR_CAPACITY, and nothing is written to image (may be NULL with
 *   image_cap 0).  GF_ERR_ARG: null pointers, a tile index outside the grid's tiles, two non-empty records of one tile, a
 *   non-empty record whose length is no multiple of 8 or below 24, decreasing offsets, facts gf_file_open would refuse (sizes
 *   < 1, n_elems < 1, an element type outside 0..3), a string of more than 65535 bytes; GF_ERR_UNSUPPORTED: n_elems > GF_MAX_ELEMS,
 *   n_codecs > 255, an unknown codec id, more than 0x7fffffff tiles.
 *   gf_file_write_block_elems_dev: blocks in DEVICE memory in (d_blocks, a HOST array of n_elems device pointers, rect, the types
 *   and rules of gf_block_write_elems_dev with n_old == 0), the file image out in device memory at d_image (8-byte aligned,
 *   image_cap bytes).  Runs on the context's stream (as gf_file_read_block_elems_dev does), ONLY ENQUEUES and never synchronises.
 *   The host emits the header record (directory positions and checksum still 0), the metadata records and the metadata directory;
 *   up to 3,072 bytes of them travel in k_file_finish's arguments, which writes them; more (large metadata) is copied to the image's
 *   front, bytes 16 and up, from a page-locked buffer of the context before the kernels (the one wait on the host, and only then: an
 *   EARLIER call's copy must have left that buffer, an event behind it); the block write's pipeline writes the records STRAIGHT INTO the image from first_record_pos
 *   on, in row-major order of the rectangle's tiles (no copy of the records); then k_file_dir_rect (bounding rectangle and the
 *   extended decision), k_file_dir_entries (the tile directory, every byte once), k_file_dir_crc (a wave per chunk of
 *   GF_FILE_CRC_CHUNK bytes) and k_file_finish (one wave: the metadata directory -- emitted whole on the host, checksum included,
 *   because its records lie in front of the tile records and their positions are known there -- copied to its place, the chunks'
 *   checksums folded in order, both positions patched into the header record, its checksum, and LAST the 16 bytes of the file
 *   head).  *d_image_bytes = the image's size, *d_file_status = GF_OK -- or, when the image does not fit image_cap (the record
 *   writer skipped a record whole, or a directory has no room), the size it needs and GF_ERR_CAPACITY: then no directory is
 *   written, bytes 0..15 are ZERO, and the image does not open.  No byte at or behind image_cap is ever written.  d_tile_indices,
 *   d_status (per tile of the rectangle of tiles) and d_codec_used (may be NULL) are the block write's; a tile with GF_ERR_BOUNDS
 *   or GF_DECLINED gets no record and the entry 0, and the file is valid without it.  The codec ids must map to a list the device
 *   record writer takes (GF_ERR_UNSUPPORTED otherwise, from the arguments alone).  GF_ERR_ARG: what gf_file_assemble and
 *   gf_block_write_elems_dev refuse, an unaligned d_image, NULL d_image_bytes / d_file_status.
 *   gf_file_write_block_elems: the same for host memory and any codec list: gf_block_write_elems, then gf_file_assemble in row-major
 *   order; for a list the device form takes, the same bytes.  Returns the first negative per-tile status, else the assembler's.
 * Not here: updating an existing file (below), versions <= 1.03, the tile cache.                                                */
#define GF_FILE_DIR_EXTENDED 1  /* flags: the tile directory in its extended form whatever the positions */
typedef struct gf_file_elem_facts {
    const char *name, *label, *description, *unit;
    int32_t continuous, has_range;
    gf_elem_range range;
} gf_file_elem_facts;
typedef struct gf_file_facts {
    gf_grid_spec grid;
    int32_t n_elems, n_codecs;
    const gf_elem_spec *elems;                 /* n_elems */
    const gf_file_elem_facts *elem_facts;      /* n_elems, or NULL */
    const char *const *codec_ids;              /* n_codecs */
    const char *product_label;
    int32_t checksum_enabled, raster_space, coordinate_system, reserved;
    double x0, y0, x1, y1, cell_size_x, cell_size_y, m2r[6], r2m[6];
    uint8_t uuid[16];
    int64_t time_modified;
} gf_file_facts;
typedef struct gf_file_metadata {
    const char *name, *description;
    const uint8_t *content;
    uint64_t content_bytes;
    int32_t record_id, type;
} gf_file_metadata;
gf_status gf_file_write_plan(const gf_file_facts *facts, const gf_file_metadata *metadata, int n_metadata, const gf_rect *rect,
                             int flags, uint64_t *first_record_pos, uint64_t *max_image_bytes);
gf_status gf_file_assemble(const gf_file_facts *facts, const gf_file_metadata *metadata, int n_metadata, int flags,
                           const uint8_t *blob, const uint64_t *offsets, const int32_t *tile_indices, size_t n_records,
                           uint8_t *image, size_t image_cap, uint64_t *image_bytes);
gf_status gf_file_write_block_elems_dev(gf_context *ctx, const gf_file_facts *facts, const gf_file_metadata *metadata,
                                        int n_metadata, const gf_rect *rect, const void *const *d_blocks, int flags,
                                        uint8_t *d_image, size_t image_cap, uint64_t *d_image_bytes, int32_t *d_file_status,
                                        int32_t *d_tile_indices, int32_t *d_status, uint8_t *d_codec_used);
gf_status gf_file_write_block_elems(gf_context *ctx, const gf_file_facts *facts, const gf_file_metadata *metadata, int n_metadata,
                                    const gf_rect *rect, const void *const *blocks, int flags, uint8_t *image, size_t image_cap,
                                    uint64_t *image_bytes, int32_t *tile_indices, int32_t *status, uint8_t *codec_used);

/* ---- GVRS files UPDATED IN PLACE: the record allocator, the free-space list, the three directories ---------------------------------
 * (gvrs/GvrsFile.java:443-483 opening for writing, :584-616 close; gvrs/RecordManager.java:218-312 fileSpaceAlloc, :314-384
 * fileSpaceDealloc, :386-490 writeTile, :864-883 writeTileDirectory, :885-903 readFreespaceDirectory, :905-989
 * writeFreeSpaceDirectory, :991-1017 writeMetadataDirectory, :451-454 the sticky extended form; gvrs/TileDirectory.java:121-191)
 * What GvrsFile(file, "rw") ... close() does: tile records stored into a file that exists.  The finished image is a pure function
 * of the old image, the records, their order and the modification time, and is the reference's byte for byte: every byte lies in
 * a live record or in a free node of the final list.
 *   THE ALLOCATOR.  A record of content c has sizeToStore = multipleOf8(c + 12) bytes.  fileSpaceAlloc takes the FIRST node in
 *   order of position whose size is exactly sizeToStore or at least sizeToStore + 32; a larger node is split and its surplus
 *   listed at position + sizeToStore.  With no such node, a last node that ends at the file's end and is smaller than sizeToStore
 *   is overwritten and the file extended; otherwise the record is appended.  fileSpaceDealloc lists the freed record by position:
 *   merged with the prior node where they touch (and then with the next, if they now touch), else with the next, else inserted.
 *   gf_file_update_begin needs no device and no context.  It takes the image gf_file_open opened, reads the free-space directory
 *   (record type 3: int32 count, per node int64 position and int32 size), the size words of the three directory records and the
 *   metadata directory record, keeps copies and holds no pointer into the image, and then frees the free-space directory record,
 *   the metadata directory record and the tile directory record in its own list, in that order, as opening for writing does.
 *   Judged before trusted: nodes ascend, neither overlap nor touch, positions and sizes are multiples of 8, a size is at least 24
 *   (NOT MIN_FREE_BLOCK_SIZE, 32: that bounds only the surplus of a split; a freed record of any size is listed, and the smallest
 *   record that can be freed is a tile record of 24 bytes), a node lies in [content_pos, image_bytes) and its own head in the
 *   image states the same size and type 0; the directory records have types 3 / 4 / 5, sizes that are multiples of 8 and end
 *   inside the image, and overlap no node; the tile directory record holds its entries; the count is one the record can hold;
 *   image_bytes is a multiple of 8.  GF_ERR_FORMAT: any of these; GF_ERR_BOUNDS: a position or size that reaches to or behind
 *   image_bytes (a truncated image); GF_ERR_ARG: null pointers, an image whose header record has another size than the opened
 *   one's.  No byte at or behind image_bytes is read.  A handle serves ONE image state: after an update, open and begin again.
 *   gf_file_update_free_list: the list after opening, positions[k] and sizes[k] of *n_nodes nodes (GF_ERR_CAPACITY with *n_nodes
 *   set when cap is smaller).
 *   gf_file_update_plan (rect NULL: the whole grid): *max_image_bytes = the old size + every tile the rectangle touches at
 *   gf_tile_record_max_bytes_elems + the three directories at their largest; *free_list_capacity = the nodes after opening + the
 *   tiles written + 3, the room a call's list needs.  Either pointer may be NULL.
 *   gf_file_update_assemble needs no device and no context.  image holds the old image in its first bytes and has image_cap
 *   bytes; records as gf_block_write_elems hands them out, applied IN THE CALLER'S ORDER as writeTile applies them: a non-empty
 *   record frees the tile's old record FIRST and is then allocated (in a file without compression, n_codecs == 0, an old record
 *   is rewritten at its place and nothing is allocated; the new record must have its size); length 0 with status GF_DECLINED
 *   (or status == NULL) frees the old record and sets the entry 0; a negative status leaves the tile untouched, record and entry.
 *   An old record is found as gf_file_tile_position finds it and its head judged (type 2, a size >= 24 that is a multiple of 8
 *   inside the image) before it is freed: else that verdict is returned.  Then close: time_modified, opened-for-writing 0, the
 *   metadata directory (the old record, allocated anew: no metadata is added or moved, so its bytes are the old ones), the tile
 *   directory over the bounding rectangle of the OLD rectangle and every tile that got a position (it only grows; an old extended
 *   directory stays extended, flags GF_FILE_DIR_EXTENDED or a content position above 1 << 35 make it so), the free-space directory
 *   (allocated for the count of nodes; counted AGAIN behind the allocation, which may have consumed one: the record is then 12
 *   bytes roomier; no node before the allocation: no record, the word is 0), every remaining node as [size][0 0 0 0][zeros]
 *   [CRC-32C of its first 8 bytes | 0], the three header words and the header checksum.  ALL OR NOTHING: *image_bytes = the size
 *   the image has or needs; with image_cap smaller it returns GF_ERR_CAPACITY and not one byte of the image is changed, as for
 *   every other refusal.  GF_ERR_ARG: what gf_file_assemble refuses of records and indices, two records for one tile, image_cap
 *   below the old size, blob inside image.  GF_ERR_UNSUPPORTED: a directory or a node of 2^31 bytes or more.
 *   DEVIATION from the reference: with compression enabled, an old record, and a new record that is not smaller than the standard
 *   form, writeTile has freed the old record and zeroed its entry (:429-432) and then writes the standard form into the freed
 *   block (:476-480) without restoring the entry: the tile is lost.  Here such a record is freed and allocated like any other.
 *   gf_file_update_records_dev: the assembler's device counterpart.  The records lie in device memory (d_blob, d_offsets
 *   [n_records + 1], d_tile_indices, d_status or NULL) and are placed into d_image (8-byte aligned, image_cap bytes, the old
 *   image in its first bytes).  Runs on the context's stream and ONLY ENQUEUES; the one wait on the host, as in
 *   gf_file_write_block_elems_dev with a long front: an EARLIER call's copies must have left the context's page-locked buffer, through
 *   which the opened list and the metadata directory travel (an event behind them).  k_update_alloc, one wave,
 *   runs the serial rules above over a position-sorted list (first fit by ballot over 64 nodes a turn, insert and delete as
 *   wave-wide shifts), in LDS where list_capacity nodes fit and in the context's scratch otherwise (list_capacity 0: the plan's
 *   number; a caller may pass a larger one), and writes nothing into the image; k_update_snapshot has copied the old directory
 *   entries aside before.  When the size needed exceeds image_cap, or an old record is refused, every later kernel sees the verdict
 *   and writes nothing: *d_file_status = GF_ERR_CAPACITY and *d_image_bytes = the size needed (or the verdict and 0), the image byte for
 *   byte as it was.  Otherwise k_update_copy lays the records in 8-byte words, k_update_dir the tile directory over the new
 *   rectangle, k_update_dir_crc its chunked checksum, k_update_fill every free node (a lane per 8-byte word across all nodes) and
 *   k_update_finish the metadata directory, the free-space directory and the header.  GF_ERR_ARG as the assembler, as far as the
 *   host can tell (device contents are judged on the device and reported in *d_file_status), an unaligned d_image.
 *   gf_file_update_block_elems_dev: a rectangle of the raster (d_blocks, rect, the types and rules of gf_block_write_elems_dev, the
 *   default ranges) into an image in DEVICE memory; tiles are written in row-major order of the rectangle's tiles; d_tile_indices,
 *   d_status and d_codec_used (may be NULL) are the block write's.  A rectangle whose four sides lie on tile seams (a side at a grid
 *   edge that cuts a tile is none: such a tile keeps its old cells beyond the grid) decodes nothing and the call only enqueues, as the records
 *   form.  Otherwise k_file_locate finds the old records of the rectangle's tiles in the image and the block write's merge takes
 *   them where they lie, an explicit end per record (a tile without a record, or with a refused entry, is an empty extent and a new
 *   tile to the merge): the call then synchronises once, as gf_block_write_elems_dev with old records does.  The records are
 *   written to a buffer of the context and laid by k_update_copy.  k_update_alloc judges the head of EVERY old record itself before
 *   it frees it (type 2, a size >= 24 that is a multiple of 8 inside the image): a wholly covered tile with a damaged body is
 *   overwritten; a tile whose entry or head is refused gets that status in d_status and stays, record and entry; a partly covered
 *   tile whose old record fails keeps the merge's status and stays.  The codec list must be one the device record writer takes
 *   (GF_ERR_UNSUPPORTED otherwise, from the arguments alone).  *d_file_status and *d_image_bytes as the records form.
 *   gf_file_update_block_elems: a rectangle of the raster into an image in HOST memory, any codec list: the old records of the
 *   rectangle's tiles are looked up and their heads judged on the host (a refused one gives its tile that status, and the tile
 *   stays), gf_block_write_elems merges the old cells of partly covered tiles, then gf_file_update_assemble in row-major order of
 *   the rectangle's tiles.  Cells are checked against the default ranges (the handle does not keep the header's).  Returns the
 *   assembler's status when it refuses the update (GF_ERR_CAPACITY: *image_bytes = the need), else the first negative per-tile status.
 *   WRITES AT SCATTERED POINTS (gf_file_update_points_elems_dev, gf_file_update_points_elems; gf_file_update_plan_tiles): what
 *   for i in 0 .. n_points - 1: for e: element[e].writeValue(rows[i], cols[i], values[e][i]) does to a file opened "rw", followed
 *   by close() (gvrs/GvrsElement.java writeValue / writeValueInt; the tile cache loads, modifies and rewrites only the tiles the
 *   cells fall in).  d_values is a HOST array of n_elems device pointers, d_values[e] of n_points items: int32 (INT), int16
 *   (SHORT), float32 (FLOAT) and float32 VALUES for an ICF element, the block write's types.  Only the tiles the points touch are
 *   decoded and written again; their count comes back in *n_tiles_touched, and max_tiles is the room of d_tile_indices,
 *   d_tile_status and (n_elems * max_tiles bytes, may be NULL) d_codec_used, which are the block write's outputs over the touched
 *   tiles in ascending tile index: d_codec_used[e * *n_tiles_touched + s].
 *   THE CELL RULE is TileElement*.setValue's, under "RANGES" and "ICF, per cell" of gf_block_write_elems_dev, and one piece of
 *   code with the block write (gvrs_file_points_store.h): the DEFAULT ranges apply (the handle does not keep the header's),
 *   Float.equals decides whether a value is the fill, an ICF's code is (int)Math.floor((double)((v - offset) * scale) + 0.5) with
 *   the saturating cast.
 *   PER POINT AND ELEMENT d_point_status[e * n_points + i], first match: GF_ERR_ARG for every element of a point outside the grid
 *   (the reference throws), and no tile is touched; the TILE'S status for every element where the point's tile cannot be
 *   rewritten -- a refused directory entry or record head (judged as an update judges it: type 2, a size >= 24 that is a multiple
 *   of 8 inside the image), a failed checksum where the file enables them, an element of the old record that did not decode to
 *   GF_OK: the status of the first such element, as in the block write's merge -- and nothing is stored; GF_ERR_BOUNDS for the
 *   (e, i) whose value is out of range, alone: nothing is stored for it, the other elements of the point still store (the
 *   reference throws from that one setValue and the earlier stores stand); else GF_OK.
 *   DUPLICATES: of several points on one cell the HIGHEST POINT INDEX WHOSE VALUE PASSED wins, per element, as the sequence
 *   gives it.  The result does not depend on timing: k_points_claim raises an owner word per pool cell to that index with
 *   atomicMax, and only behind it k_points_store lets the owners write.
 *   PER TOUCHED TILE d_tile_indices[s], d_tile_status[s], s < *n_tiles_touched, first match: the old record's failure as above
 *   (the tile stays, record and entry); GF_ERR_BOUNDS where no point stored anything into the tile (the reference sets
 *   writingRequired only in a successful store, TileElementInt.java:121: the tile is never written and stays; a tile whose stores
 *   happen to equal the old cells IS rewritten); GF_DECLINED where every element is all fill after the stores (the old record is
 *   freed and the entry set to 0, as in gf_file_update_assemble); else the record writer's verdict.  A tile the directory names no
 *   record for is a new tile: fill everywhere (cells beyond the grid's edge included), then the stores.
 *   THE FILE: the records go to the allocator in ascending tile index under the rules, the all-or-nothing rule, the
 *   *d_file_status / *d_image_bytes and the deviation for compressed files of gf_file_update_records_dev.  ONE MORE DEVIATION: the
 *   reference writes tiles in the order in which its cache evicts and flushes them, which depends on the cache's size and the
 *   access pattern; here the order is ascending tile index.
 *   More than max_tiles touched tiles: GF_ERR_CAPACITY, *n_tiles_touched holds the count, no status is written and not one byte of
 *   the image changes.  n_points == 0: GF_OK, *n_tiles_touched = 0, nothing is written and the image is left as it is -- it is
 *   NOT EVEN CLOSED ANEW (no modification time, no directories; the host form sets *image_bytes to the old size).  Points that all
 *   lie outside the grid touch no tile and the file IS closed anew.
 *   gf_file_update_points_elems_dev runs on the context's stream; the codec list must be one the device record writer takes
 *   (GF_ERR_UNSUPPORTED otherwise, from the arguments alone); old checksums are verified where the file enables them.  It
 *   SYNCHRONISES TWICE -- the read-back of the touched tiles' count, by which the host sizes the pool, and the decode of the old
 *   records (the records' pipeline's) -- and is NOT CAPTURE-SAFE.  Order: k_points_mark, k_points_rank, the count, k_file_locate
 *   over the list, k_points_heads, the records' pipeline into a tile-major pool (an ICF element as codes), k_file_status,
 *   k_points_prepare (new tiles filled), k_points_claim, k_points_store, k_points_verdict, the record writer from the pool with the
 *   verdict as its pre-status, the kernels of gf_file_update_records_dev with d_tile_status as the statuses.
 *   gf_file_update_points_elems: the same through host memory, for any codec list.  The touched tiles are gf_file_cells_tiles's;
 *   their records are looked up and their heads judged on the host, as gf_file_update_block_elems does, and staged end to end; the
 *   same device decode and store follow; a device-capable list goes on through the device record writer, any other brings tiles
 *   and verdicts back and goes through the host encoders; then gf_file_update_assemble's rules.  Its return value follows
 *   gf_file_update_block_elems: the assembler's status when it refuses the update, else the first negative per-tile status.
 *   gf_file_update_plan_tiles: gf_file_update_plan for n_tiles touched tiles in place of a rectangle (GF_ERR_ARG: more tiles than
 *   the grid has).
 *   GF_ERR_ARG / GF_ERR_UNSUPPORTED before the context or a device is looked at: null pointers (d_codec_used may be NULL), an
 *   unaligned d_image, image_cap below the old size; GF_CODEC_UNKNOWN in the list, more than 2^27 tiles in the grid, n_points or
 *   n_elems * max_tiles beyond 0x7fffffff.
 * Not here: adding, changing or removing metadata, versions <= 1.03, the tile cache and its
 * flush order, truncating a file whose last record became free (the reference does not either).                                 */
typedef struct gf_file_update gf_file_update;
gf_status gf_file_update_begin(const gf_file *f, const uint8_t *image, size_t image_bytes, gf_file_update **out);   /* host bytes */
void      gf_file_update_end(gf_file_update *u);
gf_status gf_file_update_free_list(const gf_file_update *u, uint64_t *positions, uint64_t *sizes, size_t cap, size_t *n_nodes);
gf_status gf_file_update_plan(const gf_file_update *u, const gf_rect *rect, uint64_t *max_image_bytes, uint64_t *free_list_capacity);
gf_status gf_file_update_assemble(const gf_file_update *u, uint8_t *image, size_t image_cap, const uint8_t *blob,
                                  const uint64_t *offsets, const int32_t *tile_indices, const int32_t *status, size_t n_records,
                                  int64_t time_modified, int flags, uint64_t *image_bytes);
gf_status gf_file_update_records_dev(gf_context *ctx, const gf_file_update *u, uint8_t *d_image, size_t image_cap,
                                     const uint8_t *d_blob, const uint64_t *d_offsets, const int32_t *d_tile_indices,
                                     const int32_t *d_status, size_t n_records, size_t blob_bytes, int64_t time_modified, int flags,
                                     size_t list_capacity, uint64_t *d_image_bytes, int32_t *d_file_status);
gf_status gf_file_update_block_elems_dev(gf_context *ctx, const gf_file_update *u, const gf_rect *rect, const void *const *d_blocks,
                                         int flags, int64_t time_modified, uint8_t *d_image, size_t image_cap, uint64_t *d_image_bytes,
                                         int32_t *d_file_status, int32_t *d_tile_indices, int32_t *d_status, uint8_t *d_codec_used);
gf_status gf_file_update_block_elems(gf_context *ctx, const gf_file_update *u, const gf_rect *rect, const void *const *blocks,
                                     int flags, int64_t time_modified, uint8_t *image, size_t image_cap, uint64_t *image_bytes,
                                     int32_t *tile_indices, int32_t *status, uint8_t *codec_used);
gf_status gf_file_update_plan_tiles(const gf_file_update *u, size_t n_tiles, uint64_t *max_image_bytes, uint64_t *free_list_capacity);
gf_status gf_file_update_points_elems_dev(gf_context *ctx, const gf_file_update *u, size_t n_points, const int32_t *d_rows,
                                          const int32_t *d_cols, const void *const *d_values /* HOST array of n_elems device pointers */,
                                          size_t max_tiles, int flags, int64_t time_modified, uint8_t *d_image, size_t image_cap,
                                          uint64_t *d_image_bytes, int32_t *d_file_status, int32_t *d_point_status,
                                          int32_t *d_tile_indices, int32_t *d_tile_status, uint8_t *d_codec_used /* may be NULL */,
                                          size_t *n_tiles_touched);
gf_status gf_file_update_points_elems(gf_context *ctx, const gf_file_update *u, size_t n_points, const int32_t *rows, const int32_t *cols,
                                      const void *const *values, size_t max_tiles, int flags, int64_t time_modified, uint8_t *image,
                                      size_t image_cap, uint64_t *image_bytes, int32_t *point_status, int32_t *tile_indices,
                                      int32_t *tile_status, uint8_t *codec_used /* may be NULL */, size_t *n_tiles_touched);

/* ---- GVRS files INSPECTED: every record walked and checksummed, as the file is laid out ----------------------------------------
 * (gvrs/GvrsInspector.java:213-312 inspectContent, :314-337 testRecordChecksum)
 * The one reader that goes record by record from the first byte of content to the image's end -- metadata, directories, free
 * nodes and tile records the directory no longer names included -- and answers whether the image, as a whole, is a file the
 * reference would accept.  The header has passed: the calls take an opened gf_file (gf_file_open refuses what the inspector's
 * constructor refuses); image may be other bytes than the ones opened (an updated image), with the same header record size.
 *   THE WALK: from content_pos, while fewer than image_bytes - 12 bytes lie in front of the position.  At one record, in this
 *   order: a size word of 0 ends the walk cleanly (complete); a type code outside 0..6 stops it (GF_INSPECT_BAD_RECORD_TYPE); a
 *   size word below 16 or no multiple of 8 stops it (_BAD_RECORD_SIZE); a tile record (type 2) whose index lies outside the grid's
 *   tiles stops it (_BAD_TILE_INDEX, bad_tile_index) and one larger than the standard form, (4 + 4 * n_elems + the standard tile
 *   bytes + 12 + 7) & ~7, is listed as bad and stops it (_TILE_TOO_LARGE, invalid_record_size); a record that ends behind the image
 *   stops it (_TRUNCATED); and, ONLY WHERE THE SPECIFICATION ENABLES CHECKSUMS, the CRC-32C of the record's first size - 4 bytes
 *   (a free node, type 0: of its first 8 bytes, whatever its body holds) is compared with its last word: a mismatch fails the file,
 *   lists a tile, and directly behind another mismatch stops the walk at this record (_TWO_CHECKSUM_FAILURES).  A stop fails the
 *   file, leaves complete 0 and termination_pos at the record; else termination_pos is where the walk ended.  tile_dir_passed: the
 *   CRC-32C of the record at the header's tile directory position, taken in every file (0 in a file without checksums, whose
 *   word is 0), or any tile directory record (type 5) the walk met that matched.
 *   DEVIATIONS from the reference, where it is undefined: _BAD_RECORD_SIZE (there an exception, a backward walk or one off the
 *   8-byte grid); _TRUNCATED in both modes (there EOFException with checksums, a walk past the end reported as complete
 *   without); termination_pos after a bad type code is the record's position (there it stays 16).
 *   No byte at or behind image_bytes is read.  The report counts the records up to and including the one the walk stopped at;
 *   bad_tiles is the reference's list, in file order, a tile twice where two of its records fail: the first bad_cap entries are
 *   written, n_bad_tiles is the true count.
 *   gf_file_inspect (host bytes; no device, no context): records may be NULL; with records_cap < n_records the call answers
 *   GF_ERR_CAPACITY (also in status), n_records is the number needed and nothing is written behind the capacity.  GF_ERR_ARG: null
 *   pointers, image_bytes < content_pos, a header record of another size than the opened one.  GF_ERR_FORMAT: a content_pos that
 *   is no multiple of 8.
 *   gf_file_inspect_dev: the image, the report, the list and the records in DEVICE memory; d_image is 8-byte aligned and readable
 *   to the end of the aligned 16-byte piece that holds its last byte.  Runs on the context's stream, ONLY ENQUEUES and never
 *   synchronises.  The result equals gf_file_inspect's on the same bytes, field for field.  The walk is cut at ANCHORS: the tile
 *   directory's entries (judged as gf_file_read_block_elems_dev judges them) and the header's three directory positions give, per
 *   segment of segment_bytes, the first record start known there; a lane per anchored segment walks to the next anchor.  THE CHAIN
 *   FROM content_pos IS THE AUTHORITY: a segment's walk counts only if the walk in front of it landed exactly on its anchor, and
 *   where a link does not close (a damaged size word, an entry that leads into the middle of a record) one lane walks the rest of
 *   the image from the landing point -- slow and correct, for damaged files only.  Checksums: a wave per record of up to 8 chunks
 *   of crc_chunk_bytes, a larger record chunk by chunk over many waves.  max_records: the room of the call's record list (0: the
 *   plan's default_max_records); the list takes every record up to the first structural stop, so with more of them the REPORT
 *   says status GF_ERR_CAPACITY and n_records = that count, and nothing else of it, the list or the records is valid.
 *   d_records (may be NULL) has max_records entries.  GF_ERR_ARG as above and an unaligned d_image; GF_ERR_UNSUPPORTED: more than
 *   2^31 - 2 records of room.
 *   gf_file_inspect_plan: the device form's numbers for an image of image_bytes (each pointer may be NULL).
 * Not here: versions <= 1.03, the tile records' payloads (the block reads decode them and report per tile), repairing a file,
 * GvrsInspector.summarize's text.                                                                                               */
enum { GF_INSPECT_END = 0, GF_INSPECT_BAD_TILE_INDEX = 1, GF_INSPECT_TILE_TOO_LARGE = 2, GF_INSPECT_TWO_CHECKSUM_FAILURES = 3,
       GF_INSPECT_BAD_RECORD_TYPE = 4, GF_INSPECT_BAD_RECORD_SIZE = 5, GF_INSPECT_TRUNCATED = 6 };
typedef struct gf_file_record {      /* one record as the walk met it */
    uint64_t pos;                    /* of its size word */
    uint32_t size;  int32_t type;    /* the size word; the type code (0..6 unless the walk stopped at it) */
    int32_t tile_index;              /* -1 unless type 2 */
    int32_t checksum;                /* 1 passed, 0 failed, -1 not checked (a file without checksums, a structural stop) */
} gf_file_record;
typedef struct gf_file_inspect_report {
    int32_t status;                  /* GF_OK, or GF_ERR_CAPACITY: only n_records is valid */
    int32_t failed, complete, stop;  /* stop: GF_INSPECT_* */
    int32_t bad_tile_index, invalid_record_size, tile_dir_located, tile_dir_passed;
    uint64_t termination_pos;
    uint64_t n_records, n_by_type[7], n_checksum_failures, n_bad_tiles;
} gf_file_inspect_report;
gf_status gf_file_inspect_plan(const gf_file *f, size_t image_bytes, uint64_t *segment_bytes, uint64_t *crc_chunk_bytes,
                               uint64_t *default_max_records);
gf_status gf_file_inspect(const gf_file *f, const uint8_t *image, size_t image_bytes, gf_file_inspect_report *report,
                          int32_t *bad_tiles, size_t bad_cap, gf_file_record *records, size_t records_cap);
gf_status gf_file_inspect_dev(gf_context *ctx, const gf_file *f, const uint8_t *d_image, size_t image_bytes, size_t max_records,
                              gf_file_inspect_report *d_report, int32_t *d_bad_tiles, size_t bad_cap, gf_file_record *d_records);

/* ---- thin device-memory helpers so that non-HIP hosts (JNI, ctypes) can
 *      stage data without linking the HIP runtime themselves --------------- */
gf_status gf_dev_malloc(gf_context *ctx, size_t bytes, void **d_ptr);
gf_status gf_dev_free(gf_context *ctx, void *d_ptr);
gf_status gf_dev_memset(gf_context *ctx, void *d_ptr, int value, size_t bytes);
gf_status gf_dev_upload(gf_context *ctx, void *d_dst, const void *h_src, size_t bytes);
gf_status gf_dev_download(gf_context *ctx, void *h_dst, const void *d_src, size_t bytes);

/* ---- timing of the device entry points with HIP events on `stream` ------
 * gf_timer_* bracket any sequence of *_dev calls; elapsed is in milliseconds. */
typedef struct gf_timer gf_timer;
gf_status gf_timer_create(gf_context *ctx, gf_timer **t);
void gf_timer_destroy(gf_timer *t);
gf_status gf_timer_start(gf_timer *t, void *stream);
gf_status gf_timer_stop(gf_timer *t, void *stream);
gf_status gf_timer_elapsed_ms(gf_timer *t, float *ms);   /* synchronises on the stop event */

#ifdef __cplusplus
}
#endif
#endif
