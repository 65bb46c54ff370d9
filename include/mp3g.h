/*
 * mp3g.h -- C-ABI of the MI355X-native MP3 Layer III granule-decode path.
 *
 * This library replaces the per-frame DSP seam of llehouerou/go-mp3:
 *
 *   func (f *Frame) Decode() []byte              reference internal/frame/frame.go:121-138
 *
 * i.e. requantize -> reorder -> MS/intensity stereo -> antialias -> hybrid
 * IMDCT + overlap -> frequency inversion -> 32-subband polyphase synthesis ->
 * s16le stereo PCM, for a BATCH of granules from many independent streams, on
 * a gfx950 GPU.  The bitstream parse (frame header, side info, scale factors,
 * Huffman, bit reservoir) stays on the host: the caller hands over exactly
 * the fields `Decode` reads (reference frame.go:140-688)
 * as packed granule descriptors plus int16 coefficients.
 *
 * Plain C types only: no torch, no HIP types in the signatures.  Every call
 * returns an mp3g_status (0 = OK); nothing throws across the ABI and no caller
 * pointer is retained after a call returns (cgo rule).
 *
 * Threading: a context / plan is single-threaded like mp3.Decoder
 * (reference decode.go:27-33); distinct contexts may be used concurrently.
 * Executions of one fast-mode plan (mp3g_plan_execute) must also be ordered
 * on the device: one stream, or streams synchronised between them -- its
 * launches share the plan's zone list (ABI 5).  One plan per stream for
 * concurrent launches.
 */
#ifndef MP3G_H
#define MP3G_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: mp3g_lame_toc_offset returns a status and writes the offset through an
 *    out-parameter (version 1 returned the offset); the fast-mode hot-granule
 *    fallback (no signature change).
 * 3: streaming input -- mp3g_reader + mp3g_decoder_new_reader, MP3G_ERR_READ;
 *    MP3G_FLAG_KERNEL_V1 retired.
 * 4: main-data kernel stages for high bitrates -- MP3G_HUFF_STAGE_MID /
 *    MP3G_HUFF_STAGE_WIDE flags of mp3g_huffman_execute_ex and the advice
 *    mp3g_huffman_stage_flags.
 * 5: mp3g_plan_hot_stats and MP3G_FLAG_HOT_STATS (the fast kernel's
 *    hot-granule fallback counters); a fast-mode plan owns a zone list its
 *    launches share, so executions of one plan must be stream-ordered.
 *    (Compatible additions since: the diagnostic mp3g_debug_clock_probe;
 *    float32 PCM output -- MP3G_OUT_*, mp3g_out_bytes_per_granule,
 *    mp3g_plan_execute_out and mp3g_decode_host_out; the mono downmix
 *    formats MP3G_OUT_S16_MONO / MP3G_OUT_F32_MONO and
 *    mp3g_decode_streams_into_out; sample-windowed decode into dense rows --
 *    mp3g_scan_windows, mp3g_scan_window_rows, mp3g_plan_create_windows and
 *    mp3g_plan_execute_windows; sample-rate conversion of decoded rows --
 *    mp3g_resampler_*, mp3g_resample_host, mp3g_resample_rows and
 *    mp3g_stream_rates; log-mel features of decoded rows -- mp3g_logmel_*;
 *    Kaldi filter-bank features of decoded rows -- mp3g_fbank_*; STFT and mel
 *    spectrograms of decoded rows -- mp3g_stft_*; Kaldi MFCC features of
 *    decoded rows -- mp3g_mfcc_*; per-row mean and variance normalisation --
 *    mp3g_cmvn_rows and mp3g_cmvn_host; BS.1770 integrated loudness of decoded
 *    rows and the gain stage -- mp3g_loudness_*, mp3g_gain_rows and
 *    mp3g_gain_host; true peak, momentary and short-term maxima and loudness
 *    range of decoded rows and the gain against a supplied peak --
 *    mp3g_true_peak_*, mp3g_loudness_range_*, mp3g_gain_rows_peak and
 *    mp3g_gain_host_peak; sliding-window CMN, energy VAD and voiced-frame
 *    selection of feature tensors -- mp3g_sliding_cmn_*, mp3g_vad_energy_* and
 *    mp3g_select_frames_*; variable-ratio resampling of decoded rows (speed
 *    and volume perturbation) -- mp3g_varresampler_*, mp3g_varresample_host
 *    and mp3g_varresample_rows; SpecAugment of feature tensors --
 *    mp3g_specaug_*; delta features and frame context (splicing,
 *    low-frame-rate stacking, subsampling) of feature tensors --
 *    mp3g_delta_scales, mp3g_add_deltas_* and mp3g_stack_frames_*.) */
#define MP3G_ABI_VERSION 5

/* ---- status codes ------------------------------------------------------ */
typedef enum mp3g_status {
  MP3G_OK = 0,
  MP3G_ERR_INVALID_ARGUMENT = 1, /* null pointer, bad sizes, bad plan       */
  MP3G_ERR_INVALID_GRANULE = 2,  /* descriptor field out of range (checked mode) */
  MP3G_ERR_NO_DEVICE = 3,        /* no gfx950 device / HIP init failed      */
  MP3G_ERR_DEVICE = 4,           /* HIP runtime error (see mp3g_last_error) */
  MP3G_ERR_OUT_OF_MEMORY = 5,
  MP3G_ERR_PARSE = 6,            /* host bitstream parse error (decoder API) */
  MP3G_EOF = 7,                  /* end of stream (decoder API, io.EOF)      */
  MP3G_ERR_UNSUPPORTED = 8,      /* MPEG 2.5, layer I/II, free format, ...   */
  MP3G_ERR_NO_XING_HEADER = 9,   /* lameinfo.ErrNoXingHeader                 */
  MP3G_ERR_UNEXPECTED_EOF = 10, /* io.ErrUnexpectedEOF (lameinfo.ParseFromReader) */
  MP3G_ERR_READ = 11             /* the caller's reader callback failed (decoder API;
                                    decode.go:48-63 returns a reader's error as is) */
} mp3g_status;

/* ---- boundary input: one granule descriptor ---------------------------- */
/*
 * Per-channel fields read by the DSP.  Field <- reference source:
 *   count1           sideinfo.SideInfo.Count1, set by maindata/huffman.go:451
 *   global_gain      sideinfo.go:115            scalefac_scale  sideinfo.go:151
 *   preflag          sideinfo.go:149 (MPEG-1) / maindata.go:136 (MPEG-2)
 *   win_switch_flag  sideinfo.go:117            block_type      sideinfo.go:119,143
 *   mixed_block_flag sideinfo.go:120            subblock_gain   sideinfo.go:125
 *   scalefac_l       maindata.MainData.ScalefacL[gr][ch] (maindata.go:34)
 *   scalefac_s       maindata.MainData.ScalefacS[gr][ch] (maindata.go:35)
 * 72 bytes, no padding.
 */
typedef struct mp3g_channel {
  uint16_t count1;          /* 0..576: first line of the zero region          */
  uint8_t global_gain;      /* 0..255                                         */
  uint8_t scalefac_scale;   /* 0/1                                            */
  uint8_t preflag;          /* 0/1                                            */
  uint8_t win_switch_flag;  /* 0/1                                            */
  uint8_t block_type;       /* 0..3                                           */
  uint8_t mixed_block_flag; /* 0/1                                            */
  uint8_t subblock_gain[3]; /* 0..7                                           */
  uint8_t scalefac_l[22];   /* 0..15                                          */
  uint8_t scalefac_s[13][3];/* [sfb][win], 0..15                              */
} mp3g_channel;

/*
 * One granule = half an MPEG-1 frame (or a whole MPEG-2 LSF frame).
 *   header : the raw 32-bit frameheader.FrameHeader (frameheader.go:29-137);
 *            the DSP reads lsf, sampling-frequency index, mode, mode_ext from it.
 *   gr     : granule index inside its frame (0/1), informational.
 * 160 bytes (16-byte multiple so a descriptor is ten 16-B loads).
 */
typedef struct mp3g_granule {
  uint32_t header;
  uint32_t gr;
  mp3g_channel ch[2];
  uint8_t reserved[8];
} mp3g_granule;

/* Coefficients: int16 [n_granules][2][576], the integer Huffman output that
 * the reference keeps as float32 in MainData.Is (maindata.go:36).  |x| <= 8206
 * (15 + 13 linbits).  Mono granules leave [g][1][*] unread. */
#define MP3G_LINES 576
#define MP3G_COEF_PER_GRANULE (2 * MP3G_LINES)
/* PCM: int16 [n_granules][576][2] = the bytes Decode() returns, concatenated
 * (frame.go:134: granule gr at byte 2304*gr; mono duplicated, frame.go:671-678). */
#define MP3G_PCM_BYTES_PER_GRANULE (MP3G_LINES * 2 * 2)

/* ---- output formats (mp3g_plan_execute_out / mp3g_decode_host_out /
 *      mp3g_decode_streams_into_out) ---------------------------------------
 * The stereo sample value is the same in every format and both modes.  With
 * t = sum * 32767 as the window stage computes it (frame.go:649-662),
 *   s16:   (int16)trunc(clamp(t, -32767, 32767))        (frame.go:663-669)
 *   float: f = clamp(t, -32767, 32767) * 2^-15          (no truncation)
 * so (int16)trunc(f * 32768) is exactly the s16 sample of the same plan and
 * |f| <= 32767/32768.  Mono granules write channel 0 to both channels / planes
 * (frame.go:671-678).  The exported state does not depend on the format.
 * MP3G_OUT_F32_PLANAR needs streams that do not overlap, each of fewer than
 * MP3G_PLANAR_MAX_GRANULES granules (MP3G_ERR_UNSUPPORTED otherwise).
 *
 * The mono formats hold one downmixed channel: sample i of granule g at index
 * 576 g + i, so a stream's samples are contiguous and in time order.
 *   MP3G_OUT_S16_MONO: m = (L + R) >> 1 on the s16 samples (L, R) that
 *     MP3G_OUT_S16 of the same plan writes -- an arithmetic shift (floor) of
 *     the 32-bit sum.  Exact mode stays a pure function of the reference's
 *     bytes; fast mode's +-1 per channel gives floors at most 1 apart.
 *   MP3G_OUT_F32_MONO: m = (fL + fR) * 0.5f on the float samples (fL, fR) that
 *     MP3G_OUT_F32 writes -- one float32 add rounded to nearest, then the
 *     exact halving; |m| <= 32767/32768.
 * A mono granule gives m = L, or m = fL bit for bit.  The two mono formats
 * round at different points: trunc(m * 32768) of the float sample is NOT
 * promised to equal the MP3G_OUT_S16_MONO sample (the identity above holds for
 * the stereo formats only). */
#define MP3G_OUT_S16        0u /* int16 [n_granules][576][2]: the layout above             */
#define MP3G_OUT_F32        1u /* float [n_granules][576][2]: same order, float32          */
#define MP3G_OUT_F32_PLANAR 2u /* float; stream s (first F, n granules) owns floats
                                  [F*1152, (F+n)*1152): plane ch at F*1152 + ch*n*576,
                                  n*576 samples, in time order                             */
#define MP3G_OUT_S16_MONO   3u /* int16 [n_granules][576]: (L + R) >> 1                       */
#define MP3G_OUT_F32_MONO   4u /* float [n_granules][576]: (fL + fR) * 0.5f                   */
#define MP3G_PLANAR_MAX_GRANULES 900000u /* (a plane pair is addressed with 31-bit byte offsets) */
/* Output bytes per granule of a format: 2304 / 4608 / 4608 / 1152 / 2304;
 * 0 = unknown format. */
size_t mp3g_out_bytes_per_granule(uint32_t out_format);

/* ---- cross-granule DSP state (reference Frame.store / Frame.vVec) ------- */
/* Layout identical to the reference fields (frame.go:48-49): copying a
 * Frame's state in/out is a memcpy.  12,800 bytes.  A state_in is a state a
 * decoder produced (Frame.store / vVec are only ever written by Decode): its
 * vVec blocks are V = synthNWin * S, whose 64 entries hold 33 distinct values,
 * and the one-wave kernels (fast v3, exact v4) keep only those; the workgroup
 * kernel (MP3G_FLAG_KERNEL_V2) carries all 64 of any vvec. */
typedef struct mp3g_state {
  float store[2][32][18]; /* IMDCT overlap                          */
  float vvec[2][1024];    /* polyphase FIFO, newest V block at [0:64] */
} mp3g_state;

/* ---- streams ------------------------------------------------------------ */
/* A stream is a run of consecutive granules of one MP3 stream; the granules
 * of stream s are [first_granule, first_granule + n_granules) in the granule
 * and coefficient arrays, and its PCM goes to the same granule slots of the
 * output.  State is carried inside the run exactly as frame.Read carries it
 * (frame.go:110-113). */
#define MP3G_STREAM_STATE_IN  1u /* start from state_in[s] (else zero state, = stream start / after Seek, decode.go:106-108) */
#define MP3G_STREAM_STATE_OUT 2u /* write the state after the last granule to state_out[s] */
typedef struct mp3g_stream {
  uint64_t first_granule;
  uint32_t n_granules;
  uint32_t flags;
} mp3g_stream;

/* ---- decode modes -------------------------------------------------------- */
#define MP3G_MODE_EXACT 0u   /* bit-exact vs the reference (linux/amd64 float semantics) */
#define MP3G_MODE_FAST  1u   /* reassociated fast transforms; |dPCM| <= 1 LSB            */
#define MP3G_FLAG_CHECKED 0x100u /* validate descriptor ranges on the host first      */
#define MP3G_FLAG_KERNEL_V1 0x200u /* retired in ABI 3 (the per-phase v1 cross-check kernel):
                                      mp3g_plan_create returns MP3G_ERR_UNSUPPORTED */
#define MP3G_FLAG_KERNEL_V2 0x800u /* exact mode via the workgroup v2 kernel (cross-check; the
                                      default exact kernel is v4, one wave per chunk) */
#define MP3G_FLAG_HOST_HUFFMAN 0x400u /* decoder: scale factors + Huffman on the host (mp3g_parse_*)
                                         instead of the GPU main-data kernel (cross-check) */
#define MP3G_FLAG_HOT_STATS 0x1000u /* fast-mode plans: count the hot-granule fallback's work
                                       (mp3g_plan_hot_stats; a kernel build that costs ~1.5 %) */

/* ---- library / device ---------------------------------------------------- */
int mp3g_abi_version(void);
/* Human-readable text for a status code; static storage. */
const char* mp3g_status_string(int status);
/* Last HIP/runtime error text of this thread (empty if none); static storage. */
const char* mp3g_last_error(void);
/* Number of visible gfx950 devices. */
int mp3g_device_count(int* out_count);

/* ---- checked-mode validation (host only, no GPU) ------------------------- */
/* Returns MP3G_OK or MP3G_ERR_INVALID_GRANULE and the first bad index. */
int mp3g_validate(const mp3g_granule* granules, const int16_t* coeffs,
                  uint64_t n_granules, uint64_t* bad_index);

/* ---- plans: device-resident work decomposition ---------------------------
 * A plan splits every stream into chunks processed by independent waves /
 * workgroups.  granules_per_chunk: 0 < k < 2^31 = every stream cut into
 * ceil(n / k) chunks of equal length +-1 (so at most k granules each);
 * 0 = automatic (a length from the launch-cost model, then the chunk count
 * rounded to whole rounds of resident chunks and every stream cut into
 * chunks of equal length +-1); MP3G_PLAN_CHUNKS(c) = about c chunks in total,
 * spread over the streams by length, equal lengths +-1 (c < 2^31).  Every
 * chunk holds < 2^32 granules (MP3G_ERR_UNSUPPORTED otherwise).  A chunk that does
 * not start a stream re-derives its entry state from the two preceding
 * granules (bit-identical to serial decode; DESIGN.md "halo").  The plan lives
 * on `device` and can be executed many times (graph-capturable). */
#define MP3G_PLAN_CHUNKS(c) (0x80000000u | (uint32_t)(c))
typedef struct mp3g_plan mp3g_plan;
int mp3g_plan_create(int device, const mp3g_stream* streams, uint32_t n_streams,
                     uint32_t granules_per_chunk, uint32_t mode, mp3g_plan** out_plan);
int mp3g_plan_destroy(mp3g_plan* plan);
/* Number of chunks (= workgroups launched) and granules incl. halo work. */
int mp3g_plan_info(const mp3g_plan* plan, uint64_t* n_chunks, uint64_t* n_granules,
                   uint64_t* n_halo_granules);

/* Asynchronous execution on device-resident buffers.  All pointers are device
 * pointers; `hip_stream` is a hipStream_t (NULL = default stream).  state_in /
 * state_out may be NULL when no stream of the plan uses the flag.
 * Fast mode (ABI 5): a launch's hot zones go through a zone list owned by the
 * plan and emptied by the launch itself (graph replays are fine), so two
 * executions of ONE plan must not overlap on the device -- issue them on one
 * stream or synchronise the streams; concurrent launches need a plan each.
 * If the zone launch cannot be enqueued, the list is reset on the stream
 * before the error is returned (the next execution starts clean). */
int mp3g_plan_execute(mp3g_plan* plan, const mp3g_granule* d_granules,
                      const int16_t* d_coeffs, const mp3g_state* d_state_in,
                      mp3g_state* d_state_out, int16_t* d_pcm, void* hip_stream);
/* The same with the output format chosen per call (MP3G_OUT_*): d_out holds
 * mp3g_out_bytes_per_granule(out_format) bytes per granule slot.
 * mp3g_plan_execute is the MP3G_OUT_S16 case.  An unknown format is
 * MP3G_ERR_INVALID_ARGUMENT (checked before any device call); any format but
 * MP3G_OUT_S16 on an MP3G_FLAG_KERNEL_V2 plan is MP3G_ERR_UNSUPPORTED (the
 * one-wave kernels, fast v3 and exact v4, write floats and the mono downmix
 * straight from the window's registers; the cross-check kernel stays s16
 * stereo).  No reference counterpart: go-mp3's
 * Decode returns s16 bytes only (frame.go:121-137). */
int mp3g_plan_execute_out(mp3g_plan* plan, const mp3g_granule* d_granules,
                          const int16_t* d_coeffs, const mp3g_state* d_state_in,
                          mp3g_state* d_state_out, void* d_out, uint32_t out_format,
                          void* hip_stream);

/* Standalone polyphase synthesis: go-mp3's subbandSynthesis
 * (internal/frame/frame.go:630-688, called per channel at frame.go:133) over
 * the granules of a fast-mode plan, without the stages before it.
 * d_lines: float32 [n_granules][2][576], the frequency-inverted hybrid output
 * that subbandSynthesis reads (MainData.Is after frame.go:132; mono granules
 * leave [g][1][*] unread).  PCM as mp3g_plan_execute (+-1 LSB, fast mode).
 * State: vvec carried as in mp3g_plan_execute; state_out.store is
 * state_in.store (or zero), since this stage does not touch it. */
int mp3g_plan_synth_execute(mp3g_plan* plan, const mp3g_granule* d_granules,
                            const float* d_lines, const mp3g_state* d_state_in,
                            mp3g_state* d_state_out, int16_t* d_pcm, void* hip_stream);

/* Fast-mode plans: the work of the hot-granule fallback (granules whose
 * hybrid output exceeds the fast transforms' magnitude bound are decoded
 * again in the reference's operation order), summed over
 * the plan's launches since creation or the last reset, for plans created
 * with MP3G_FLAG_HOT_STATS (others: always 0).  out4[0]: granules whose PCM
 * that pass rewrites; out4[1]: hot zones (runs of such granules); out4[2]: hot
 * granules the fast pass flagged; out4[3]: granules re-run inside a chunk's
 * own wave -- always 0 since the zone list holds every chunk's zones (kept
 * for ABI 5 layout).
 * Synchronises the device; reset != 0 zeroes the counters after reading.
 * A fast-mode plan's launches share its zone list (emptied by each launch
 * itself: graph replays are fine): executions of one plan must be ordered
 * (one stream, or synchronised between streams).  No reference
 * counterpart: go-mp3 has one arithmetic (frame.go:140-688). */
int mp3g_plan_hot_stats(mp3g_plan* plan, uint64_t* out4, int reset);

/* ---- synchronous host-buffer decode (the cgo drop-in entry) --------------
 * Copies the batch to `device`, decodes it and copies PCM (and state_out)
 * back before returning.  Equivalent to calling Frame.Decode on every frame of
 * every stream in order.  mode = MP3G_MODE_* | optional MP3G_FLAG_CHECKED. */
int mp3g_decode_host(int device, const mp3g_granule* granules, const int16_t* coeffs,
                     uint64_t n_granules, const mp3g_stream* streams, uint32_t n_streams,
                     const mp3g_state* state_in, mp3g_state* state_out, int16_t* pcm,
                     uint32_t mode);
/* The same with an output format (MP3G_OUT_*): `out` holds
 * n_granules * mp3g_out_bytes_per_granule(out_format) bytes; mp3g_decode_host
 * is the MP3G_OUT_S16 case. */
int mp3g_decode_host_out(int device, const mp3g_granule* granules, const int16_t* coeffs,
                         uint64_t n_granules, const mp3g_stream* streams, uint32_t n_streams,
                         const mp3g_state* state_in, mp3g_state* state_out, void* out,
                         uint32_t out_format, uint32_t mode);

/* ---- host bitstream parse (CPU only) -----------------
 * The part of go-mp3's frame.Read that feeds Decode: tags (source.go:42-83),
 * sync search + header (frameheader.go:279-328), side info (sideinfo.go),
 * bit reservoir (maindata.go:290-323), scale factors and Huffman decoding
 * (maindata.go:119-288, maindata/huffman.go:27-138).  Output buffers are
 * allocated by the library (free with mp3g_free).  *end_status is MP3G_EOF
 * when the stream ended the way decode.go maps to io.EOF, MP3G_ERR_PARSE for
 * any other frame.Read error, MP3G_ERR_UNSUPPORTED where the reference would
 * panic; the granules of every frame before that point are returned. */
int mp3g_parse_stream(const uint8_t* data, size_t len, mp3g_granule** granules, int16_t** coeffs,
                      uint64_t* n_granules, int* end_status);
/* Many independent streams on n_threads host threads (0 = all cores); the
 * stream table describes where each stream's granules landed. */
int mp3g_parse_streams(uint32_t n_streams, const uint8_t* const* datas, const size_t* lens, int n_threads,
                       mp3g_granule** granules, int16_t** coeffs, uint64_t* n_granules, mp3g_stream* streams,
                       int* end_status);
void mp3g_free(void* p);

/* ---- main-data decode on the GPU --------------------
 * Splits frame.Read (frame.go:67-115) at the bit reservoir:
 *   host   (mp3g_scan_streams): tags, sync search, header, side info and the
 *          reservoir resolution -- sequential but byte-level, no Huffman;
 *   device (mp3g_huffman_execute): scale factors (maindata.go:119-288) and
 *          Huffman decoding (maindata/huffman.go:27-138, huffman/huffman.go:
 *          348-419) of every (granule, channel) in parallel, completing the
 *          granule descriptors and writing the int16 coefficients that
 *          mp3g_plan_execute consumes.
 * The result is byte-identical to mp3g_parse_streams.  The main data of each
 * stream is concatenated into one byte buffer; frame f's bit buffer (the
 * reference's `prev.Tail(main_data_begin) ++ buf`, or `prev ++ buf` on a
 * reservoir underflow, maindata.go:290-323) is always a suffix of that
 * concatenation ending at bit_end, so jobs address it with absolute bit
 * positions.
 *
 * One job per (granule, channel), jobs[2*g + ch]; 48 bytes. */
#define MP3G_SF_NONE 0        /* channel absent (mono): zero coefficients      */
#define MP3G_SF_MPEG1_LONG 1  /* maindata.go:233-279 (scfsi copies from gr 0) */
#define MP3G_SF_MPEG1_SHORT 2 /* maindata.go:221-231                          */
#define MP3G_SF_MPEG1_MIXED 3 /* maindata.go:207-220                          */
#define MP3G_SF_MPEG2_LONG 4  /* maindata.go:132-172, 22 scale factors        */
#define MP3G_SF_MPEG2_SHORT 5 /* maindata.go:173-179, 39 scale factors        */
typedef struct mp3g_hjob {
  uint64_t part2_start;     /* absolute bit position of the scale factors (maindata.go:202) */
  uint64_t bit_end;         /* end of the frame's main-data bits: reads at/after it yield 0
                               and do not advance (bits.go:45-77) */
  uint32_t scf0_delta;      /* MPEG-1 granule 1 with scfsi: granule 0's part2_start is
                               part2_start - scf0_delta */
  uint16_t part2_3_length;  /* sideinfo.go:114 */
  uint16_t big_values;      /* <= 288 (more is a frame error, found by the scan) */
  uint16_t region1_start;   /* lines (maindata/huffman.go:39-64) */
  uint16_t region2_start;
  uint8_t table_select[3];
  uint8_t count1_table;     /* count1table_select */
  uint8_t sf_kind;          /* MP3G_SF_* */
  uint8_t scfsi;            /* granule 1: bit k = scale-factor part k copied from granule 0 */
  uint8_t slen[4];          /* bits per scale factor: MPEG-1 {slen1, slen2}; MPEG-2 per part */
  uint8_t nsf[4];           /* MPEG-2: scale factors per part (ISO 13818-3 Table 6) */
  uint8_t sf0_kind;         /* granule 0's sf_kind and slen (for the scfsi copy) */
  uint8_t sf0_slen[2];
  uint8_t reserved[3];
} mp3g_hjob;

/* Host scan of many streams on n_threads host threads (0 = all cores).  The
 * scan owns its buffers until mp3g_scan_free; mp3g_scan_buffers returns:
 *   granules   [n_granules] descriptors with the side-info fields set (scale
 *              factors and count1 are written by mp3g_huffman_execute)
 *   jobs       [2 * n_granules]
 *   main_data  [main_data_bytes] (incl. 16 zero bytes of padding)
 *   streams    [n_streams] where each stream's granules landed
 *   end_status [n_streams] as mp3g_parse_streams.
 * A frame the reference rejects (frame.Read error or panic) ends its stream
 * exactly where mp3g_parse_streams ends it. */
typedef struct mp3g_scan mp3g_scan;
int mp3g_scan_streams(uint32_t n_streams, const uint8_t* const* datas, const size_t* lens, int n_threads,
                      mp3g_scan** out);
int mp3g_scan_buffers(const mp3g_scan* scan, uint64_t* n_granules, uint64_t* main_data_bytes,
                      const mp3g_granule** granules, const mp3g_hjob** jobs, const uint8_t** main_data,
                      const mp3g_stream** streams, const int** end_status);
void mp3g_scan_free(mp3g_scan* scan);

/* Device decode of the 2 * n_granules jobs (device pointers; d_granules holds
 * the scan's descriptors and is completed in place).  Asynchronous on
 * hip_stream (NULL = default stream). */
int mp3g_huffman_execute(int device, const mp3g_hjob* d_jobs, uint64_t n_granules, const uint8_t* d_main_data,
                         mp3g_granule* d_granules, int16_t* d_coeffs, void* hip_stream);
/* The same with flags.  MP3G_HUFF_ROWS_COUNT1: each coefficient row is
 * written only up to its count1 plus padding (the zero tail is left as it
 * was): what the default plan kernels (MP3G_MODE_FAST, and MP3G_MODE_EXACT
 * without MP3G_FLAG_KERNEL_V2) read, since lines at and above count1
 * are zero (maindata/huffman.go:127-134).  The batch and decoder APIs use it
 * for those modes (c3 main-data kernel -13 %). */
#define MP3G_HUFF_ROWS_COUNT1 1u
/* Main-data stage per 256-job block (ABI 4): by default 28 KB of LDS (16
 * waves per CU); MP3G_HUFF_STAGE_MID 42 KB (12 waves per CU);
 * MP3G_HUFF_STAGE_WIDE 68 KB (8 waves per CU).  A block whose main data does
 * not fit its stage reads it from global memory, which is slower: 256 jobs
 * span ~25 KB at 128 kbps, ~40 KB at 192, ~67 KB at 320.
 * mp3g_huffman_stage_flags tells which suits a batch. */
#define MP3G_HUFF_STAGE_WIDE 2u
#define MP3G_HUFF_STAGE_MID 4u
int mp3g_huffman_execute_ex(int device, const mp3g_hjob* d_jobs, uint64_t n_granules, const uint8_t* d_main_data,
                            mp3g_granule* d_granules, int16_t* d_coeffs, uint32_t flags, void* hip_stream);
/* Host-side advice for mp3g_huffman_execute_ex: the stage (0,
 * MP3G_HUFF_STAGE_MID or MP3G_HUFF_STAGE_WIDE) of least modelled time for the
 * batch's 256-job blocks, from their main-data spans (each block staged when
 * it fits, read from global memory otherwise; the stage's waves per CU).
 * `jobs`: the scan's jobs (host memory, 2 * n_granules). */
uint32_t mp3g_huffman_stage_flags(const mp3g_hjob* jobs, uint64_t n_granules);

/* Bitstreams in, PCM out (the batch drop-in): scan on the host, Huffman + DSP
 * on `device`.  *pcm (library-allocated, free with mp3g_free) holds
 * n_granules blocks of 576 stereo s16 samples; streams / end_status as
 * mp3g_parse_streams. */
int mp3g_decode_streams(int device, uint32_t n_streams, const uint8_t* const* datas, const size_t* lens,
                        int n_threads, uint32_t mode, int16_t** pcm, uint64_t* n_granules,
                        mp3g_stream* streams, int* end_status);

/* The same into caller memory, pipelined: the streams are decoded in groups
 * and each group's host scan overlaps the transfers and kernels of the group
 * before it.  The output layout comes from a header-only pre-pass: stream k
 * starts at block streams[k].first_granule of `pcm` (576 stereo s16 samples
 * per block); a stream its side info ends early (a parse error or a
 * reference panic after its last good frame) decodes its n_granules blocks
 * and leaves the rest of its range zero.  `pcm` (host memory; pinned memory
 * keeps the device-to-host copies at PCIe speed and asynchronous) must hold
 * pcm_cap_granules blocks; if that is too few, nothing is decoded and the
 * call returns MP3G_ERR_INVALID_ARGUMENT with *n_granules = the blocks
 * needed.  n_groups = 0 picks the group count. */
int mp3g_decode_streams_into(int device, uint32_t n_streams, const uint8_t* const* datas, const size_t* lens,
                             int n_threads, uint32_t mode, uint32_t n_groups, int16_t* pcm,
                             uint64_t pcm_cap_granules, uint64_t* n_granules, mp3g_stream* streams,
                             int* end_status);

/* The same with an output format (MP3G_OUT_*, all of them): `out` holds
 * out_cap_granules * mp3g_out_bytes_per_granule(out_format) bytes, and stream
 * k's output starts at byte streams[k].first_granule *
 * mp3g_out_bytes_per_granule(out_format) of it (MP3G_OUT_F32_PLANAR: its two
 * planes inside that range, as above).  A stream that ends early leaves the
 * rest of its range zero in every format.  An unknown format is
 * MP3G_ERR_INVALID_ARGUMENT before any device call.
 * mp3g_decode_streams_into is the MP3G_OUT_S16 case. */
int mp3g_decode_streams_into_out(int device, uint32_t n_streams, const uint8_t* const* datas, const size_t* lens,
                                 int n_threads, uint32_t mode, uint32_t n_groups, void* out, uint32_t out_format,
                                 uint64_t out_cap_granules, uint64_t* n_granules, mp3g_stream* streams,
                                 int* end_status);

/* mp3g_decode_streams_into keeps its staging (page-locked) and device
 * buffers per device between calls; this frees them (idle sets only). */
void mp3g_release_cached_buffers(void);

/* ---- sample-windowed decode into dense rows -------------------------------
 * A batch of B clips of T samples, one per stream, without decoding the files
 * around them.  For stream k a window is (start, n_samples): `start` is a
 * per-channel sample index into the stream's full decode (the sequence
 * mp3g_scan_streams + mp3g_plan_execute_out produce, untrimmed); row k of the
 * output receives samples [start, start + n_valid), n_valid = min(n_samples,
 * available - start) clamped at 0, and the plan writes only those samples:
 * the rest of the rows is the caller's (zero it first for a padded batch).
 *   MP3G_OUT_F32_PLANAR  float [B][2][T]  (channel stride T, row stride 2 T;
 *                        mono granules write channel 0 to both planes)
 *   MP3G_OUT_F32_MONO    float [B][T]
 * Every written float is bit-identical to the same sample of the full decode
 * of the stream in the same format and mode (fast mode: to the fast-mode full
 * decode, hot zones included).
 *
 * Host scan.  Only the frames a window needs are scanned: granules [h, hi) of
 * the stream, lo = start / 576, hi = ceil((start + n_samples) / 576) capped at
 * the stream's granules, and h <= lo the plans' replay start ("halo": two
 * granules back, further back to the second-latest stereo granule before lo
 * -- the only one when there is one -- so that channel 1's state is right
 * across mono granules; lo - 2 when no stereo granule precedes lo, where
 * channel 1's state is zero in either decode).  Granules [h, lo) are decoded
 * with PCM off.  The scanner restarts with an empty bit reservoir at a frame p
 * <= frame(h), chosen so that frames p .. frame(h) - 1 hold at least 511 bytes
 * of main data (p = 0 when the walk back reaches the first frame): their main
 * data is appended, no jobs are emitted for them, and from frame(h) on every
 * bit buffer equals the full scan's (main_data_begin <= 511).  A stream's
 * main data in the scan is therefore its window frames' own plus less than 511
 * bytes and one frame's (<= 1,500 bytes): the file is not copied.
 *
 * Difference from the full decode: frames in front of frame p are only
 * header-walked, with the checks of the header-only pre-pass (sync search,
 * version, layer, frame and main-data sizes) -- as the reference's Seek trusts
 * the header walk of ensureFrameStartsAndLength (decode.go:154-216).  A side
 * info-level error in such a frame (which ends the full decode there) is not
 * seen.  From frame p on a frame the reference rejects ends the stream at
 * that frame with the end_status of the full scan; n_valid then counts the
 * samples before that frame.  end_status is MP3G_OK when the window was
 * filled before the stream's end was reached.
 *
 * MP3G_WINDOW_GAPLESS: the header walk goes to the stream's end, the first
 * frame's Xing / Info / LAME tag is read, `start` counts from the first kept
 * sample of mp3g_lame_trim and n_valid is capped by its count.  A stream
 * without a tag behaves as if the flag were off. */
#define MP3G_WINDOW_GAPLESS 1u
#define MP3G_WINDOW_MAX_SAMPLES (1u << 26) /* n_samples and T (rows are addressed with 30-bit byte offsets) */
typedef struct mp3g_window {
  uint64_t start;     /* first sample, per channel */
  uint32_t n_samples; /* samples wanted (<= the T of the plan) */
  uint32_t flags;     /* MP3G_WINDOW_* */
} mp3g_window;
/* Where stream k's window lies in its decoded run (the scan's stream table
 * describes that run, granules [h, hi)): `lead` = lo - h granules decoded with
 * PCM off, `skip` = start mod 576 samples of granule lo in front of the
 * window, n_valid samples written.  A window past the stream's end has an
 * empty run and an all-zero row. */
typedef struct mp3g_window_row {
  uint32_t lead;
  uint32_t skip;
  uint32_t n_valid;
  uint32_t reserved;
} mp3g_window_row;
/* Returns an ordinary mp3g_scan (mp3g_scan_buffers / mp3g_scan_free). */
int mp3g_scan_windows(uint32_t n_streams, const uint8_t* const* datas, const size_t* lens,
                      const mp3g_window* windows, int n_threads, mp3g_scan** out);
/* The per-stream layout of a windowed scan ([n_streams], owned by the scan);
 * MP3G_ERR_INVALID_ARGUMENT for a scan mp3g_scan_streams made. */
int mp3g_scan_window_rows(const mp3g_scan* scan, const mp3g_window_row** rows);

/* A plan over windowed runs: streams / rows as the windowed scan returns them
 * (n of each), T = the row length in samples (every n_valid <= T <=
 * MP3G_WINDOW_MAX_SAMPLES).  Chunks cover only granules [first + lead, first
 * + n) of each stream -- its first chunk replays the lead as any chunk that
 * does not start its stream replays its halo -- and the automatic chunk
 * length is modelled on those lengths; mp3g_plan_info counts the lead in
 * n_halo_granules.  mode: MP3G_MODE_EXACT or MP3G_MODE_FAST (|
 * MP3G_FLAG_HOT_STATS); MP3G_FLAG_KERNEL_V2 is MP3G_ERR_UNSUPPORTED (checked
 * before any device call).  Such a plan runs with mp3g_plan_execute_windows
 * only. */
int mp3g_plan_create_windows(int device, const mp3g_stream* streams, const mp3g_window_row* rows,
                             uint32_t n_streams, uint32_t T, uint32_t granules_per_chunk, uint32_t mode,
                             mp3g_plan** out_plan);
/* d_out: float [n_streams][2][T] (MP3G_OUT_F32_PLANAR) or [n_streams][T]
 * (MP3G_OUT_F32_MONO); only the n_valid samples of each row (and plane) are
 * written.  An unknown format is MP3G_ERR_INVALID_ARGUMENT, the other known
 * formats MP3G_ERR_UNSUPPORTED, both before any device call.  Asynchronous on
 * hip_stream; executions of one plan must be stream-ordered (as
 * mp3g_plan_execute). */
int mp3g_plan_execute_windows(mp3g_plan* plan, const mp3g_granule* d_granules, const int16_t* d_coeffs,
                              void* d_out, uint32_t out_format, void* hip_stream);

/* ---- sample-rate conversion of decoded rows --------------------------------
 * A polyphase windowed-sinc resampler for the float rows the windowed decode
 * delivers: MP3 streams come at 32 / 44.1 / 48 kHz (MPEG-1) or 16 / 22.05 /
 * 24 kHz (MPEG-2) and a model wants one rate.  No reference counterpart:
 * go-mp3 delivers every stream at its own rate (decode.go:137-140).
 *
 * Filter.  For source rate fi and target rate fo: g = gcd(fi, fo), M = fi / g,
 * L = fo / g, c = rolloff * min(1, L / M) (cutoff relative to the source
 * Nyquist), W = ceil(zeros / c) (half width in source samples) and
 *   h[r][k] = c sinc(c t) kaiser(t / W),  t = k - (W - 1) - r / L,
 *   sinc(u) = sin(pi u) / (pi u),  kaiser(u) = I0(beta sqrt(1 - u^2)) / I0(beta)
 * for r in [0, L), k in [0, 2W), computed in float64 and rounded once to
 * float32; no per-phase normalisation.  zeros outside 1..64 or a table of more
 * than MP3G_RESAMPLE_MAX_TAPS entries is MP3G_ERR_UNSUPPORTED, a rate <= 0 or a
 * rolloff outside (0, 1] MP3G_ERR_INVALID_ARGUMENT, before any device call.
 *
 * Signal.  x is zero outside [0, N).  For output n, (q, r) = divmod(n M, L)
 * (64-bit; n M / L < 2^63) and
 *   acc = +0.0f;  for k = 0 .. 2W-1: acc = fmaf(h[r][k], x[q - W + 1 + k], acc)
 *   y[n] = acc
 * -- ONE float32 FMA chain in ascending k.  The order is part of the contract:
 * the device call equals mp3g_resample_host bit for bit, whatever the tiling.
 * (Taps on samples outside [0, N) may be skipped: the accumulator starts at +0
 * and never becomes -0.)  y has ceil(N L / M) samples.  fi == fo is a copy:
 * y = x, L = M = 1, W = 0, no taps. */
#define MP3G_RESAMPLE_MAX_TAPS (1u << 18)
#define MP3G_RESAMPLE_FAST_ZEROS 16 /* resampy's kaiser_fast */
#define MP3G_RESAMPLE_FAST_ROLLOFF 0.85
#define MP3G_RESAMPLE_FAST_BETA 8.555504641634386
#define MP3G_RESAMPLE_BEST_ZEROS 64 /* resampy's kaiser_best */
#define MP3G_RESAMPLE_BEST_ROLLOFF 0.9475937167399596
#define MP3G_RESAMPLE_BEST_BETA 14.769656459379492
typedef struct mp3g_resampler mp3g_resampler;
/* Builds the table; device >= 0 also uploads it to that device (once), device
 * = -1 makes a host-only object (mp3g_resample_host, mp3g_resampler_info). */
int mp3g_resampler_create(int device, int fi, int fo, int zeros, double rolloff, double beta,
                          mp3g_resampler** out);
void mp3g_resampler_free(mp3g_resampler* r);
/* L, M, W, the host table float [L][2W] (owned by the resampler; NULL for a
 * copy) and the device call's output tile length (any may be NULL). */
int mp3g_resampler_info(const mp3g_resampler* r, uint32_t* L, uint32_t* M, uint32_t* W, const float** taps,
                        uint32_t* tile);
/* The definition above in plain C++ (the reference the device call equals):
 * source sample j is src[j - src_origin] for src_origin <= j < src_origin +
 * n_src and 0 otherwise; writes y[out_start .. out_start + n_out) to `out`. */
int mp3g_resample_host(const mp3g_resampler* r, const float* src, uint64_t src_origin, uint64_t n_src,
                       uint64_t out_start, uint64_t n_out, float* out);
/* One row of the device call: outputs y[out_start, out_start + n_out) of the
 * signal whose samples [src_origin, src_origin + n_src) are row src_row of
 * the source (zero elsewhere), to the first n_out floats of row out_row of the
 * output.  32 bytes. */
typedef struct mp3g_resample_row {
  uint64_t out_start;
  uint64_t src_origin;
  uint32_t src_row;
  uint32_t out_row;
  uint32_t n_src; /* <= src_stride */
  uint32_t n_out; /* <= out_stride */
} mp3g_resample_row;
/* d_src: float [*][n_channels][src_stride], d_out: float [*][n_channels]
 * [out_stride], n_channels 1 or 2 (every plane of a row is resampled alike);
 * d_rows: n_rows descriptors.  All three are device pointers and the launch
 * shape depends on none of their contents: asynchronous on hip_stream and
 * graph-capturable.  Writes the n_out samples of each row and plane and
 * nothing else; a row whose n_out exceeds out_stride is cut at out_stride. */
int mp3g_resample_rows(const mp3g_resampler* r, const float* d_src, uint32_t src_stride, float* d_out,
                       uint32_t out_stride, uint32_t n_channels, const mp3g_resample_row* d_rows,
                       uint32_t n_rows, void* hip_stream);
/* The sample rate of each stream's first valid frame (after tags and the sync
 * search, as mp3g_decoder_info reports it; found by the header walk, no side
 * info parsed) and its channel count (1 / 2; either output may be NULL).  A
 * stream without a valid frame gets 0 and 0. */
int mp3g_stream_rates(uint32_t n_streams, const uint8_t* const* datas, const size_t* lens, int n_threads,
                      int* rates, int* channels);

/* ---- variable-ratio resampling of decoded rows ------------------------------
 * Speed and volume perturbation (sox `speed`, Kaldi's 3-way speed and volume
 * recipes, a factor drawn per utterance): a resampler whose ratio and gain are
 * fields of the row descriptor, so ONE launch serves rows of any ratios.  No
 * reference counterpart (go-mp3 delivers every stream at its own rate).
 *
 * Object.  One prototype table that depends on no ratio: P = precision (5..9),
 * Z = zeros << P and, for i = 0..Z,
 *   f(v) = sinc(v) kaiser(v / zeros),  F[i] = f(i / 2^P),  F[Z] = 0,
 *   D[i] = f((i + 1) / 2^P) - f(i / 2^P),  D[Z] = 0
 * (sinc, kaiser and I0 as in the section above), computed in float64 and
 * rounded once to float32; R = floor(rolloff 2^P) is fixed at creation.  zeros
 * outside 1..64 or precision outside 5..9 is MP3G_ERR_UNSUPPORTED, a rolloff
 * outside (0, 1] or R == 0 MP3G_ERR_INVALID_ARGUMENT, before any device call.
 * The presets are the MP3G_RESAMPLE_FAST_* / _BEST_* triples.
 *
 * Row.  num / den is source samples per output sample, 1 <= num, den < 2^31
 * (not necessarily reduced); gain multiplies the output.
 *
 * Cutoff, in integers only: I = R for num <= den, else floor(R den / num) (64
 * bits); c = I / 2^P (exact in float32); Wr = ceil(Z / I) is the row's half
 * width in source samples.  The quantised cutoff is at most 2^-P below
 * rolloff min(1, den / num): the price of an interpolation fraction that is
 * constant along a wing (resampy's resample_f loop, with its truncated
 * index_step made consistent between the filter's scale and its gain).
 *
 * Signal.  x is zero outside [0, N).  For output n, (q, r) = divmod(n num, den)
 * (64-bit; n num / den < 2^62).
 *   left wing:  source j = q - k, k >= 0, table index iL(k) = oL + I k with
 *     (oL, remL) = divmod(I r, den), etaL = (float)((double)remL / (double)den)
 *   right wing: source j = q + 1 + k, index iR(k) = oR + I k with
 *     (oR, remR) = divmod(I (den - r), den), etaR likewise
 * A tap exists while its index is < Z; its weight is w = fmaf(eta, D[i], F[i]).
 *   acc = +0.0f;  acc = fmaf(w, x[j], acc) over all existing taps in ASCENDING j
 *   (the left wing from its farthest tap inwards, then the right wing outwards)
 *   y[n] = (c * acc) * gain      -- two float32 multiplications, in that order
 * Taps on samples outside [0, N) are skipped.  The order is part of the
 * contract: the device call equals mp3g_varresample_host bit for bit, whatever
 * the tiling.  y has ceil(N den / num) samples.  num == den is a copy times
 * gain: y[n] = x[n] * gain, no filter (-0 stays -0 at gain = 1). */
typedef struct mp3g_varresampler mp3g_varresampler;
/* Builds the table; device >= 0 also uploads it to that device (once), device
 * = -1 makes a host-only object (mp3g_varresample_host, mp3g_varresampler_info). */
int mp3g_varresampler_create(int device, int zeros, double rolloff, double beta, int precision,
                             mp3g_varresampler** out);
void mp3g_varresampler_free(mp3g_varresampler* r);
/* P, Z, R, the host table float [Z + 1][2] of (F[i], D[i]) pairs (owned by the
 * object), the device call's output tile length, and the floats of its source
 * stage -- a tile's span of (tile - 1) num / den + 2 Wr samples is staged when
 * it is at most stage / n_channels (any may be NULL). */
int mp3g_varresampler_info(const mp3g_varresampler* r, uint32_t* precision, uint32_t* Z, uint32_t* R,
                           const float** table, uint32_t* tile, uint32_t* stage);
/* The definition above in plain C++ for one row (the reference the device call
 * equals): source sample j is src[j - src_origin] for src_origin <= j <
 * src_origin + n_src and 0 otherwise; writes y[out_start .. out_start + n_out)
 * to `out`.  num or den outside [1, 2^31), or a ratio with I == 0 (num > R den),
 * is MP3G_ERR_INVALID_ARGUMENT. */
int mp3g_varresample_host(const mp3g_varresampler* r, const float* src, uint64_t src_origin, uint64_t n_src,
                          uint64_t out_start, uint64_t n_out, float* out, uint32_t num, uint32_t den, float gain);
/* One row of the device call: mp3g_resample_row's fields, the ratio and the
 * gain.  48 bytes. */
typedef struct mp3g_varresample_row {
  uint64_t out_start;
  uint64_t src_origin;
  uint32_t src_row;
  uint32_t out_row;
  uint32_t n_src; /* <= src_stride */
  uint32_t n_out; /* <= out_stride */
  uint32_t num;   /* source samples per output sample: num / den */
  uint32_t den;
  float gain;
  uint32_t reserved; /* 0 */
} mp3g_varresample_row;
/* Buffers as mp3g_resample_rows.  ONE launch for all rows, whatever their
 * ratios; its shape depends on n_rows, out_stride and n_channels alone:
 * asynchronous on hip_stream and graph-capturable.  Writes the n_out samples
 * of each row and plane and nothing else (n_out is cut at out_stride, n_src at
 * src_stride); the kernel stays within the strides for any descriptor
 * contents, and a row with den == 0, num == 0 or I == 0 gets +0 in its n_out
 * samples.  Strides and n_rows are below 2^31. */
int mp3g_varresample_rows(const mp3g_varresampler* r, const float* d_src, uint32_t src_stride, float* d_out,
                          uint32_t out_stride, uint32_t n_channels, const mp3g_varresample_row* d_rows,
                          uint32_t n_rows, void* hip_stream);

/* ---- log-mel features of decoded rows ---------------------------------------
 * The input of a speech model from the float rows of the windowed, resampled
 * decode: STFT power, mel filter bank, log10 and (MP3G_LOGMEL_CLAMP) Whisper's
 * dynamic-range normalisation.  Every feature is a fixed sequence of float32
 * operations, so the device call equals mp3g_logmel_host bit for bit.  No
 * reference counterpart (go-mp3 delivers samples).
 *
 * Parameters.  n_fft a multiple of 4 in [16, 1024], 1 <= hop <= n_fft, n_mels
 * in 1..128, rate > 0, 0 <= fmin < fmax <= rate / 2 (fmax = 0 means rate / 2);
 * K = n_fft / 2 + 1 bins.  A value that is not positive, an unknown flag, hop >
 * n_fft or an fmin / fmax outside those relations is MP3G_ERR_INVALID_ARGUMENT;
 * an n_fft or n_mels outside the supported range MP3G_ERR_UNSUPPORTED; both
 * before any device call, with *out = NULL.
 *
 * Framing.  One row is a float32 signal x[0, T) (a plane of the dense batch,
 * its zero padding included).  With MP3G_LOGMEL_CENTER pad = n_fft / 2 and
 * frame f reads xr[f hop - pad + n], n = 0 .. n_fft - 1, where xr is x
 * reflected about both ends (xr[-i] = x[i], xr[T - 1 + i] = x[T - 1 - i]:
 * torch.stft(center=True, pad_mode="reflect")); it needs T > pad and has
 * frames 0 .. T / hop.  Without it pad = 0 and the frames are 0 ..
 * (T - n_fft) / hop.  The caller asks for n_frames <= that count (Whisper:
 * T / hop, which drops the last).
 *
 * Tables, computed in float64 and rounded once to float32:
 *   w[n] = 0.5 - 0.5 cos(2 pi n / n_fft)           (periodic Hann)
 *   Cw[k][n] = w[n] cos(2 pi ((k n) mod n_fft) / n_fft),  Sw[k][n] = -w[n] sin(..)
 *   Wm[m][k]: librosa.filters.mel's defaults -- Slaney's scale, triangles
 *   between n_mels + 2 points equally spaced in mel, each scaled by 2 / (its
 *   width in Hz); filter m's non-zero entries are k in [lo_m, hi_m].
 *
 * Features, all float32:
 *   re = im = +0;  for n = 0 .. n_fft-1: re = fmaf(Cw[k][n], xr[..], re), im alike
 *   p[k] = fmaf(re, re, im * im)                   (the product rounded first)
 *   mel = +0;  for k = lo_m .. hi_m: mel = fmaf(Wm[m][k], p[k], mel)
 *   y[m][f] = mp3g_log10f(max(mel, 1e-10f))
 * -- each sum ONE FMA chain in ascending order; the order is part of the
 * contract.  mp3g_log10f (go-mp3_amd/csrc/logmel_log10.h) is built from integer
 * operations and explicit FMAs only and compiled by host and device alike; it
 * is within half an ulp of its result + 2^-45 of log10.  MP3G_LOGMEL_CLAMP then
 * takes mx = the maximum of y over the n_mels x n_frames features of the row
 * and plane and replaces y by (max(y, mx - 8.0f) + 4.0f) * 0.25f.
 *
 * Domain: finite samples with |x| <= 2^20; float32 subnormals are kept.
 * Output: float [row][plane][n_mels][frame_stride], n_frames features written
 * per mel row, nothing else. */
#define MP3G_LOGMEL_CENTER 1u
#define MP3G_LOGMEL_CLAMP 2u
#define MP3G_LOGMEL_MIN_FFT 16
#define MP3G_LOGMEL_MAX_FFT 1024
#define MP3G_LOGMEL_MAX_MELS 128
typedef struct mp3g_logmel mp3g_logmel;
/* Builds the tables; device >= 0 also uploads them to that device (once),
 * device = -1 makes a host-only object. */
int mp3g_logmel_create(int device, int rate, int n_fft, int hop, int n_mels, double fmin, double fmax,
                       uint32_t flags, mp3g_logmel** out);
void mp3g_logmel_free(mp3g_logmel* lm);
/* K, the host tables Cw and Sw float [K][n_fft] and Wm float [n_mels][K], the
 * supports uint32 [n_mels][2] = lo_m, hi_m (lo > hi: an empty filter) -- all
 * owned by the object -- and the frames a workgroup of the device call
 * produces (any may be NULL). */
int mp3g_logmel_info(const mp3g_logmel* lm, uint32_t* K, const float** cw, const float** sw, const float** wm,
                     const uint32_t** support, uint32_t* tile_frames);
/* The frames a row of T samples has (0: none, or T >= 2^62). */
uint64_t mp3g_logmel_frames(const mp3g_logmel* lm, uint64_t T);
/* The definition above in plain C++ (the reference the device call equals):
 * out[m * frame_stride + f] for m < n_mels, f < n_frames <= mp3g_logmel_frames. */
int mp3g_logmel_host(const mp3g_logmel* lm, const float* x, uint64_t T, uint64_t n_frames, float* out,
                     uint64_t frame_stride);
/* d_src: float [n_rows][n_planes][T]; d_out: float [n_rows][n_planes][n_mels]
 * [frame_stride].  Both are device pointers and the launch shape depends on
 * none of their contents: asynchronous on hip_stream and graph-capturable.
 * T < 2^31; n_frames <= mp3g_logmel_frames(lm, T), frame_stride >= n_frames.
 * Executions of one MP3G_LOGMEL_CLAMP object must be ordered on the device (one
 * stream, or streams synchronised between them): they share the object's
 * buffer of row maxima.  One object per stream for concurrent launches. */
int mp3g_logmel_execute(const mp3g_logmel* lm, const float* d_src, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                        float* d_out, uint32_t n_frames, uint32_t frame_stride, void* hip_stream);
/* Test hook: y[i] = mp3g_log10f(x[i]) (normal positive finite x). */
void mp3g_logmel_log10f(const float* x, uint64_t n, float* y);

/* ---- Kaldi filter-bank features of decoded rows ------------------------------
 * The other family of speech front ends: Kaldi's compute-fbank-feats (what
 * torchaudio.compliance.kaldi.fbank restates), the input of the Conformer /
 * Zipformer, Paraformer, AST and speaker-embedding models.  It differs from the
 * log-mel features above in more than parameters: every frame is processed on
 * its own before the window (DC removal, pre-emphasis), the FFT length is the
 * window rounded up to a power of two, the mel bank is unnormalised triangles
 * in the 1127 ln(1 + f / 700) domain, the logarithm is natural and floored at
 * float32 epsilon, and the features are time-major.  Every feature is a fixed
 * sequence of float32 operations, so the device call equals mp3g_fbank_host bit
 * for bit.  No reference counterpart (go-mp3 delivers samples).
 *
 * Parameters.  rate > 0; the window length N in samples, any integer in [16,
 * 1024]; 1 <= hop <= N; n_mels in 1..128; low_freq and high_freq with Kaldi's
 * meaning (high_freq <= 0 means rate / 2 + high_freq; then 0 <= low < high <=
 * rate / 2); preemph in [0, 1]; scale finite and > 0 (Kaldi models read
 * int16-range samples: 32768; the product with a sample is exact when scale is
 * a power of two); window one of MP3G_FBANK_WINDOW_*; flags MP3G_FBANK_REMOVE_DC
 * and MP3G_FBANK_SNIP_EDGES.  P is the smallest power of two >= N (P <= 1024)
 * and K = P / 2 bins: the Nyquist bin carries no weight in Kaldi's bank and is
 * not computed.  A value that is not positive, an unknown flag or window, a
 * violated relation or a non-finite parameter is MP3G_ERR_INVALID_ARGUMENT; an N
 * or n_mels outside the supported range MP3G_ERR_UNSUPPORTED; both before any
 * device call, with *out = NULL.
 * Not offered: dither (random, so not reproducible), the energy column, VTLN,
 * subtract_mean, and magnitude (non-power) or non-log output (the energy is
 * mp3g_mfcc's coefficient 0, subtract_mean is mp3g_cmvn_rows; both below).
 *
 * Framing.  One row is a float32 signal x[0, T) (a plane of the dense batch,
 * its zero padding included).  A row with T < N has no frames, in both modes.
 * With MP3G_FBANK_SNIP_EDGES there are F = 1 + (T - N) / hop frames and frame f
 * starts at f hop.  Without it F = (T + hop / 2) / hop (integer divisions),
 * frame f starts at f hop + hop / 2 - N / 2 and reads xr, x reflected Kaldi's
 * way: xr[j] = x[-j - 1] for j < 0 and x[2 T - 1 - j] for j >= T (the edge
 * sample is repeated, unlike the log-mel reflection).
 *
 * Tables, computed in float64 and rounded once to float32:
 *   w[n], n = 0 .. N-1, a = 2 pi n / (N - 1): POVEY (0.5 - 0.5 cos a)^0.85,
 *   HAMMING 0.54 - 0.46 cos a, HANNING 0.5 - 0.5 cos a, RECTANGULAR 1
 *   Cw[k][n] = w[n] cos(2 pi ((k n) mod P) / P),  Sw[k][n] = -w[n] sin(..),  k < K
 *   Wm[m][k]: Kaldi's get_mel_banks without VTLN -- mel(f) = 1127 ln(1 + f / 700),
 *   d = (mel(high) - mel(low)) / (n_mels + 1), left = mel(low) + m d, centre =
 *   left + d, right = centre + d, mk = mel(k rate / P), Wm = max(0, min((mk -
 *   left) / d, (right - mk) / d)); no area normalisation; filter m's non-zero
 *   entries are k in [lo_m, hi_m] (lo > hi: an empty filter)
 *   rN = float32(1 / N)
 *
 * Features, all float32, start = the frame's first index:
 *   s[n] = scale * xr[start + n]                            n = 0 .. N-1
 *   sum = +0; sum = fmaf(s[n], 1.0f, sum), n ascending; mean = sum * rN
 *   d[n] = fmaf(mean, -1.0f, s[n])          (MP3G_FBANK_REMOVE_DC; else d = s)
 *   e[0] = fmaf(-preemph, d[0], d[0]);  e[n] = fmaf(-preemph, d[n-1], d[n])
 *   re = im = +0;  for n = 0 .. N-1: re = fmaf(Cw[k][n], e[n], re), im alike
 *   p[k] = fmaf(re, re, im * im)                 (the product rounded first)
 *   mel = +0;  for k = lo_m .. hi_m: mel = fmaf(Wm[m][k], p[k], mel)
 *   y[f][m] = mp3g_logf(max(mel, 0x1p-23f))
 * -- each sum ONE FMA chain in ascending order; the order is part of the
 * contract.  preemph = 0 still runs the e step (fmaf(-0, d, d) is d for finite
 * d).  mp3g_logf (go-mp3_amd/csrc/fbank_log.h) is built like mp3g_log10f from
 * integer operations and explicit FMAs only and compiled by host and device
 * alike; it is within one ulp of the float32 nearest to ln (faithful).
 *
 * Domain: finite samples with |scale x| <= 2^20; float32 subnormals are kept.
 * Output: float [row][plane][n_frames][mel_stride], mel_stride >= n_mels: time-
 * major, Kaldi's layout.  n_mels features are written per frame, nothing else. */
#define MP3G_FBANK_REMOVE_DC 1u
#define MP3G_FBANK_SNIP_EDGES 2u
#define MP3G_FBANK_WINDOW_POVEY 0
#define MP3G_FBANK_WINDOW_HAMMING 1
#define MP3G_FBANK_WINDOW_HANNING 2
#define MP3G_FBANK_WINDOW_RECTANGULAR 3
#define MP3G_FBANK_MIN_WINDOW 16
#define MP3G_FBANK_MAX_WINDOW 1024
#define MP3G_FBANK_MAX_MELS 128
typedef struct mp3g_fbank mp3g_fbank;
/* Builds the tables; device >= 0 also uploads them to that device (once),
 * device = -1 makes a host-only object. */
int mp3g_fbank_create(int device, int rate, int N, int hop, int n_mels, double low_freq, double high_freq,
                      double preemph, double scale, int window, uint32_t flags, mp3g_fbank** out);
void mp3g_fbank_free(mp3g_fbank* fb);
/* P, K, the host tables Cw and Sw float [K][N] and Wm float [n_mels][K], the
 * supports uint32 [n_mels][2] = lo_m, hi_m, the window w float [N] -- all owned
 * by the object -- and the frames a workgroup of the device call produces (any
 * may be NULL). */
int mp3g_fbank_info(const mp3g_fbank* fb, uint32_t* P, uint32_t* K, const float** cw, const float** sw,
                    const float** wm, const uint32_t** support, const float** w, uint32_t* tile_frames);
/* The frames a row of T samples has (0: none, or T >= 2^62). */
uint64_t mp3g_fbank_frames(const mp3g_fbank* fb, uint64_t T);
/* The definition above in plain C++ (the reference the device call equals):
 * out[f * mel_stride + m] for f < n_frames <= mp3g_fbank_frames, m < n_mels. */
int mp3g_fbank_host(const mp3g_fbank* fb, const float* x, uint64_t T, uint64_t n_frames, float* out,
                    uint64_t mel_stride);
/* d_src: float [n_rows][n_planes][T]; d_out: float [n_rows][n_planes][n_frames]
 * [mel_stride].  Both are device pointers and the launch shape depends on none
 * of their contents: one launch, asynchronous on hip_stream and graph-
 * capturable.  T < 2^31; n_frames <= mp3g_fbank_frames(fb, T), mel_stride >=
 * n_mels. */
int mp3g_fbank_execute(const mp3g_fbank* fb, const float* d_src, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                       float* d_out, uint32_t n_frames, uint32_t mel_stride, void* hip_stream);
/* Test hook: y[i] = mp3g_logf(x[i]) (normal positive finite x). */
void mp3g_fbank_logf(const float* x, uint64_t n, float* y);

/* ---- Kaldi MFCC features of decoded rows --------------------------------------
 * Kaldi's compute-mfcc-feats (what torchaudio.compliance.kaldi.mfcc restates):
 * the filter-bank features above through a DCT and a cepstral lifter, with the
 * frame's log energy as coefficient 0 -- the input of the x-vector / ECAPA
 * speaker recipes, of language-ID systems and of the GMM recipes.  An mp3g_mfcc
 * owns an mp3g_fbank built by mp3g_fbank_create from its front-end parameters
 * and adds to it.  Every feature is a fixed sequence of float32 operations, so
 * the device call equals mp3g_mfcc_host bit for bit.  No reference counterpart.
 *
 * Parameters.  Everything mp3g_fbank_create takes, with the same checks and the
 * same status codes; n_ceps in 1..n_mels; cepstral_lifter Q finite and >= 0 (0:
 * no lifter); energy_floor 0 or a normal positive float32; flags
 * MP3G_FBANK_REMOVE_DC, MP3G_FBANK_SNIP_EDGES, MP3G_MFCC_USE_ENERGY and
 * MP3G_MFCC_RAW_ENERGY (without USE_ENERGY it is accepted and has no effect).  A
 * violated relation, a non-finite value or an unknown flag is
 * MP3G_ERR_INVALID_ARGUMENT, a range the front end does not support
 * MP3G_ERR_UNSUPPORTED; both before any device call, with *out = NULL.
 * Not offered: htk_compat (the energy stays coefficient 0), dither and VTLN.
 *
 * Tables, computed in float64 and rounded once to float32, M = n_mels:
 *   D[i][m], i < n_ceps: Kaldi's ComputeDctMatrix -- D[0][m] = sqrt(1 / M),
 *   D[i][m] = sqrt(2 / M) cos(pi / M (m + 0.5) i)
 *   lift[i] = 1 + 0.5 Q sin(pi i / Q); exactly 1.0f when Q = 0
 *   lef = mp3g_logf(energy_floor) when the floor is positive
 *
 * Features, all float32.  s, mean, d, e, re, im, p and mel are mp3g_fbank's and
 *   L[f][m] = mp3g_logf(max(mel, 0x1p-23f))
 * is, with the same front-end parameters, mp3g_fbank_host's output bit for bit.
 * The log energy, only with MP3G_MFCC_USE_ENERGY:
 *   v[n] = d[n]                      (MP3G_MFCC_RAW_ENERGY: before pre-emphasis
 *                                     and window, after DC removal)
 *   v[n] = w[n] * e[n]               (otherwise; one rounded product)
 *   en = +0; en = fmaf(v[n], v[n], en), n ascending over 0 .. N-1
 *   le = mp3g_logf(max(en, 0x1p-23f));  if energy_floor > 0 and le < lef: le = lef
 * The cepstra:
 *   c = +0; c = fmaf(D[i][m], L[f][m], c), m ascending over 0 .. M-1
 *   y[f][i] = c * lift[i]            (one rounded product, also when Q = 0)
 *   y[f][0] = le                     (MP3G_MFCC_USE_ENERGY: after the lifter,
 *                                     in place of c0, as in Kaldi)
 * -- each sum ONE FMA chain in ascending order; the order is part of the
 * contract.  Framing, frame counts, reflection and the sample domain are
 * mp3g_fbank's.
 * Output: float [row][plane][n_frames][cep_stride], cep_stride >= n_ceps, time-
 * major.  n_ceps values are written per frame, nothing else. */
#define MP3G_MFCC_USE_ENERGY 4u
#define MP3G_MFCC_RAW_ENERGY 8u
typedef struct mp3g_mfcc mp3g_mfcc;
/* Builds the tables and the owned mp3g_fbank; device >= 0 also uploads them to
 * that device (once), device = -1 makes a host-only object. */
int mp3g_mfcc_create(int device, int rate, int N, int hop, int n_mels, int n_ceps, double low_freq, double high_freq,
                     double preemph, double scale, double cepstral_lifter, double energy_floor, int window,
                     uint32_t flags, mp3g_mfcc** out);
void mp3g_mfcc_free(mp3g_mfcc* mf);
/* The owned front end (for mp3g_fbank_info; not to be freed), n_ceps, D float
 * [n_ceps][n_mels] and lift float [n_ceps] -- owned by the object --, lef (0
 * without a floor) and whether the device call keeps D in LDS (any may be
 * NULL). */
int mp3g_mfcc_info(const mp3g_mfcc* mf, const mp3g_fbank** fbank, uint32_t* n_ceps, const float** dct,
                   const float** lifter, float* log_energy_floor, uint32_t* dct_in_lds);
/* The frames a row of T samples has: mp3g_fbank_frames of the front end. */
uint64_t mp3g_mfcc_frames(const mp3g_mfcc* mf, uint64_t T);
/* The definition above in plain C++ (the reference the device call equals):
 * out[f * cep_stride + i] for f < n_frames <= mp3g_mfcc_frames, i < n_ceps. */
int mp3g_mfcc_host(const mp3g_mfcc* mf, const float* x, uint64_t T, uint64_t n_frames, float* out,
                   uint64_t cep_stride);
/* d_src: float [n_rows][n_planes][T]; d_out: float [n_rows][n_planes][n_frames]
 * [cep_stride].  Both are device pointers and the launch shape depends on none
 * of their contents: one launch, asynchronous on hip_stream and graph-
 * capturable.  T < 2^31; n_frames <= mp3g_mfcc_frames(mf, T), cep_stride >=
 * n_ceps. */
int mp3g_mfcc_execute(const mp3g_mfcc* mf, const float* d_src, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                      float* d_out, uint32_t n_frames, uint32_t cep_stride, void* hip_stream);

/* ---- Per-row mean and variance normalisation -----------------------------------
 * Kaldi's per-utterance apply-cmvn (subtract_mean, with MP3G_CMVN_NORM_VARS also
 * the variance) on a time-major feature tensor float [n_rows][n_planes]
 * [n_frames][stride] -- the output of mp3g_fbank_execute or mp3g_mfcc_execute --
 * in place.  The batch is zero-padded, so every row brings its own frame count.
 * For each plane of row r, column c < n_cols and n = min(lengths[r], n_frames);
 * n = 0 writes nothing; otherwise, in double:
 *   sum = 0; sum += (double)x[f][c], f ascending over 0 .. n-1;  mean = sum / n
 *   with NORM_VARS: sq = 0; sq += (double)x[f][c] * (double)x[f][c] (the product
 *   of two converted floats is exact);  var = sq / n - mean * mean (the product
 *   rounded first);  vf = max((float)var, 1e-20f);  scale = 1.0f / sqrtf(vf)
 *   y[f][c] = (float)((double)x[f][c] - mean), with NORM_VARS times scale (one
 *   rounded float32 product), for f < n
 * Frames f >= n and columns >= n_cols are not touched.  The device call equals
 * the host call bit for bit.  stride < n_cols, an unknown flag or a null pointer
 * with work to do is MP3G_ERR_INVALID_ARGUMENT; no rows, planes, frames or
 * columns is MP3G_OK with nothing done.  mp3g_cmvn_rows: d_feats and d_lengths
 * (uint32 [n_rows]) are device pointers; one launch, asynchronous on hip_stream
 * and graph-capturable. */
#define MP3G_CMVN_NORM_VARS 1u
int mp3g_cmvn_rows(int device, float* d_feats, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
                   uint32_t stride, uint32_t n_cols, const uint32_t* d_lengths, uint32_t flags, void* hip_stream);
int mp3g_cmvn_host(float* feats, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames, uint32_t stride,
                   uint32_t n_cols, const uint32_t* lengths, uint32_t flags);

/* ---- Sliding-window CMN, energy VAD and voiced-frame selection -----------------
 * The three steps Kaldi's speaker recipes (voxceleb, sre16, callhome) run between
 * compute-mfcc-feats and the network -- apply-cmvn-sliding (what
 * torchaudio.functional.sliding_window_cmn computes), compute-vad-energy and
 * select-voiced-frames -- on a time-major feature tensor float [n_rows][n_planes]
 * [n_frames][stride] of which n_cols <= stride columns are live: the output of
 * mp3g_fbank_execute or mp3g_mfcc_execute.  lengths: uint32 [n_rows], one frame
 * count per row as for mp3g_cmvn_rows; below, n = min(lengths[r], n_frames).
 * Every device call (*_rows: device pointers throughout) equals its host call
 * bit for bit, is one launch whose shape depends on no buffer's contents,
 * asynchronous on hip_stream, and allocates nothing.
 *
 * Sliding-window CMN.  Out of place (a frame reads neighbours up to a window
 * away): out has in's shape and must not overlap it.  cmn_window = W >= 1,
 * min_window >= 1, flags MP3G_SCMN_CENTER and MP3G_SCMN_NORM_VARS.  The window
 * [s, e) of frame t < n, in signed integers:
 *   centred: s = t - W / 2 (integer division), e = s + W
 *   otherwise: s = t - W, e = t + 1
 *   if s < 0: e -= s, s = 0
 *   if not centred and e > t: e = max(t + 1, min_window)
 *   if e > n: s -= e - n, e = n, s = max(s, 0)
 * so 0 <= s <= t < e <= n, and s and e never decrease in t (they grow by at most
 * one per frame).  The sums, per plane and column, in ONE written-down order:
 * frames are cut into blocks of K = 32;
 *   b[j]  = the float64 sum of (double)x[f] over block j, f ascending from +0.0
 *   Bp[j] = the float64 sum of b[0..j), ascending from +0.0
 *   P[f]  = Bp[f / K] + (block f / K's partial sum up to but excluding f,
 *           ascending from +0.0),  0 <= f <= n
 *   P2 the same over the exact products (double)x * (double)x
 *   mean = (P[e] - P[s]) / (e - s);  y[t] = (float)((double)x[t] - mean)
 *   with NORM_VARS: var = (P2[e] - P2[s]) / (e - s) - mean * mean (the product
 *   rounded first);  scale = 1.0f / sqrtf(fmaxf((float)var, 1e-10f)) -- Kaldi's
 *   floor for this tool, not mp3g_cmvn_rows' 1e-20;  y[t] *= scale, one rounded
 *   float32 product.  A window of one frame gives +0.
 * Frames f >= n (a row with n = 0: all of them) have their n_cols live columns
 * copied from in; words at columns >= n_cols are never written.  stride < n_cols,
 * an unknown flag, W = 0, min_window = 0, out overlapping in or a null pointer
 * with work to do is MP3G_ERR_INVALID_ARGUMENT before any device call; no rows,
 * planes, frames or columns is MP3G_OK with nothing done.  The device call keeps
 * a row's block sums in LDS: n_frames above 20,479 with NORM_VARS, 40,959
 * without, is MP3G_ERR_UNSUPPORTED.
 *
 * Energy VAD on column col < n_cols (the log energy: coefficient 0 of an MFCC
 * made with MP3G_MFCC_USE_ENERGY), per plane:
 *   thr = energy_threshold exactly when energy_mean_scale == 0 (the column is
 *   then not summed); otherwise thr = (float)((double)energy_threshold +
 *   (double)energy_mean_scale * (P[n] / (double)n)), P the blocked sum above
 *   for t < n: den = the number of t2 in [t - c, t + c] within [0, n), c =
 *   frames_context; num = how many of those have x[t2] > thr (a float32
 *   comparison);  voiced[t] = (float)num >= (float)den * proportion_threshold,
 *   the product in float32, rounded once (Kaldi's BaseFloat)
 * voiced: uint8 [n_rows][n_planes][n_frames], frames t >= n written 0; counts:
 * uint32 [n_rows][n_planes], the ones of each plane (n = 0: 0).  A frame costs
 * min(2 c + 1, n) comparisons.  col >= n_cols, stride < n_cols or a null pointer
 * with work to do is MP3G_ERR_INVALID_ARGUMENT.
 *
 * Selection.  out: float [n_rows][n_planes][n_frames_out][stride_out], stride_out
 * >= n_cols, not overlapping in.  With m = min(the number of t < n with
 * voiced[t] != 0, n_frames_out): out[j][0..n_cols) is a copy of the j-th such
 * frame for j < m and +0 for m <= j < n_frames_out, so the batch stays dense and
 * zero-padded; words at columns >= n_cols are never written; lengths_out
 * (uint32 [n_rows][n_planes]) = m. */
#define MP3G_SCMN_CENTER 1u
#define MP3G_SCMN_NORM_VARS 2u
int mp3g_sliding_cmn_rows(int device, const float* d_in, float* d_out, uint32_t n_rows, uint32_t n_planes,
                          uint32_t n_frames, uint32_t stride, uint32_t n_cols, const uint32_t* d_lengths,
                          uint32_t cmn_window, uint32_t min_window, uint32_t flags, void* hip_stream);
int mp3g_sliding_cmn_host(const float* in, float* out, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
                          uint32_t stride, uint32_t n_cols, const uint32_t* lengths, uint32_t cmn_window,
                          uint32_t min_window, uint32_t flags);
int mp3g_vad_energy_rows(int device, const float* d_feats, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
                         uint32_t stride, uint32_t n_cols, uint32_t col, const uint32_t* d_lengths,
                         float energy_threshold, float energy_mean_scale, float proportion_threshold,
                         uint32_t frames_context, uint8_t* d_voiced, uint32_t* d_counts, void* hip_stream);
int mp3g_vad_energy_host(const float* feats, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames, uint32_t stride,
                         uint32_t n_cols, uint32_t col, const uint32_t* lengths, float energy_threshold,
                         float energy_mean_scale, float proportion_threshold, uint32_t frames_context,
                         uint8_t* voiced, uint32_t* counts);
int mp3g_select_frames_rows(int device, const float* d_in, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
                            uint32_t stride, uint32_t n_cols, const uint8_t* d_voiced, const uint32_t* d_lengths,
                            float* d_out, uint32_t n_frames_out, uint32_t stride_out, uint32_t* d_lengths_out,
                            void* hip_stream);
int mp3g_select_frames_host(const float* in, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames, uint32_t stride,
                            uint32_t n_cols, const uint8_t* voiced, const uint32_t* lengths, float* out,
                            uint32_t n_frames_out, uint32_t stride_out, uint32_t* lengths_out);

/* ---- SpecAugment: time warp, frequency and time masks ---------------------------
 * The augmentation the ASR recipes apply to the features (Park et al. 2019;
 * ESPnet's SpecAug, lhotse's and icefall's SpecAugment, wenet's spec_aug,
 * torchaudio's TimeMasking and FrequencyMasking) on a feature tensor of either
 * layout:
 *   time-major, float [n_rows][n_planes][n_frames][stride] with n_bins <= stride
 *   live columns: the output of mp3g_fbank_execute or mp3g_mfcc_execute;
 *   with MP3G_SPECAUG_FREQ_MAJOR, float [n_rows][n_planes][n_bins][stride] with
 *   n_frames <= stride live frames: the output of mp3g_logmel_execute or the mel
 *   output of mp3g_stft_execute.
 * lengths: uint32 [n_rows], one frame count per row as for mp3g_cmvn_rows; below,
 * n = min(lengths[r], n_frames).  The random parameters are the caller's: one
 * mp3g_specaug_row per row (176 bytes; both planes of a row share it), which the
 * _rows call reads from device memory, so no launch shape depends on them.
 *
 * Nothing in a descriptor can make a call fail.  A mask [start, start + width) is
 * clipped to [0, n) (time) or [0, n_bins) (frequency), the end formed in 64 bits:
 * a width of 0 or a start at or past the end masks nothing.  n_time above
 * MP3G_SPECAUG_MAX_TIME_MASKS (16) and n_freq above MP3G_SPECAUG_MAX_FREQ_MASKS
 * (4) count as the maxima.  A warp with warp_center or warp_to outside [1, n - 1]
 * is no warp.
 *
 * Order: first the warp, then the union of all masks; time masks count frames
 * AFTER the warp.  Every mask of a (row, plane) writes the same fill, so the order
 * among masks does not matter.
 *
 * Time warp (MP3G_SPECAUG_WARP; ESPnet's and lhotse's time_warp): with c =
 * warp_center and w = warp_to, source frames [0, c) are stretched onto
 * destination frames [0, w) and [c, n) onto [w, n), each segment on its own by
 * what torch.nn.functional.interpolate(mode="bicubic", align_corners=False)
 * computes when the other axis keeps its size: a 4-tap cubic convolution along
 * time with A = -0.75.  The position is stated in integers.  For a segment of
 * n_in source frames mapped onto n_out destination frames, destination frame j of
 * the segment:
 *   p = (2 j + 1) n_in - n_out, in signed 64 bits
 *   i = floor(p / (2 n_out)), which is >= -1;  r = p - i * 2 n_out
 *   t = (float)r / (float)(2 n_out), one float32 division of two exact operands
 *   (n_frames <= 2^22)
 *   c1(x) = fmaf(fmaf(1.25f, x, -2.25f), x * x, 1.0f), x * x rounded
 *   c2(x) = fmaf(fmaf(fmaf(-0.75f, x, 3.75f), x, -6.0f), x, 3.0f)
 *   w0 = c2(t + 1.0f), w1 = c1(t), w2 = c1(1.0f - t), w3 = c2(2.0f - t)
 *   x0 .. x3 = source frames i - 1 .. i + 2, each clamped to [0, n_in - 1] OF ITS
 *   OWN SEGMENT
 *   y = fmaf(w3, x3, fmaf(w2, x2, fmaf(w1, x1, w0 * x0)))
 * A segment with n_in == n_out has t = 0 and weights 0, 1, 0, 0: it reproduces
 * its input's values (a -0 may come out as +0).  A row without a warp is copied,
 * not interpolated: -0 and any NaN payload survive.
 *
 * Fill: fill_value, written as given; or with MP3G_SPECAUG_FILL_MEAN the mean of
 * the row's live region of the INPUT, per plane, in one written-down order that
 * is the same for both layouts:
 *   s[f] = the float64 sum of (double)x[f][b] over b ascending from +0.0, f < n
 *   total = the blocked sum of s[0..n), exactly P[n] of the sliding-window CMN
 *   above with K = 32
 *   fill = (float)(total / ((double)n * (double)n_bins));  n = 0: +0.0
 * The fills are also written to fills, float [n_rows][n_planes], which the caller
 * provides; the buffer is required with this flag.
 *
 * Frames f >= n have their live words copied from in; words at columns or frames
 * past the live count are never written.  With MP3G_SPECAUG_WARP the call is out
 * of place and out must not overlap in.  Without it the warp fields are ignored
 * and out == in exactly is allowed: only the masked words are then written, and
 * no other word is read or written.  A partial overlap is refused.  A stride
 * below the live count, an unknown flag, a null pointer with work to do or a bad
 * overlap is MP3G_ERR_INVALID_ARGUMENT before any device call; n_frames above
 * 2^22 with the warp flag is MP3G_ERR_UNSUPPORTED; no rows, planes, frames or
 * bins is MP3G_OK with nothing done (with FILL_MEAN the fills are written, +0.0).
 * mp3g_specaug_rows: device pointers throughout; one launch, or two with
 * FILL_MEAN (the sums first), whose shapes depend on no buffer's contents,
 * asynchronous on hip_stream; the library allocates nothing.  Its output, the
 * fills included, equals mp3g_specaug_host's bit for bit. */
#define MP3G_SPECAUG_FREQ_MAJOR 1u
#define MP3G_SPECAUG_WARP 2u
#define MP3G_SPECAUG_FILL_MEAN 4u
#define MP3G_SPECAUG_MAX_TIME_MASKS 16
#define MP3G_SPECAUG_MAX_FREQ_MASKS 4
typedef struct mp3g_specaug_row {
  uint32_t warp_center, warp_to; /* frames [0,c) -> [0,w), [c,n) -> [w,n); see above */
  uint32_t n_time, n_freq;       /* masks in use; values above the maxima count as the maxima */
  uint32_t time[MP3G_SPECAUG_MAX_TIME_MASKS][2]; /* start, width, in frames AFTER the warp */
  uint32_t freq[MP3G_SPECAUG_MAX_FREQ_MASKS][2]; /* start, width, in bins */
} mp3g_specaug_row;
int mp3g_specaug_rows(int device, const float* d_in, float* d_out, uint32_t n_rows, uint32_t n_planes,
                      uint32_t n_frames, uint32_t n_bins, uint32_t stride, const uint32_t* d_lengths,
                      const mp3g_specaug_row* d_desc, uint32_t flags, float fill_value, float* d_fill,
                      void* hip_stream);
int mp3g_specaug_host(const float* in, float* out, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
                      uint32_t n_bins, uint32_t stride, const uint32_t* lengths, const mp3g_specaug_row* desc,
                      uint32_t flags, float fill_value, float* fills);

/* ---- Delta features and frame context --------------------------------------------
 * The steps that sit between the features and the model in the recipes: Kaldi's
 * add-deltas, and one gather that is splice-feats, FunASR's low-frame-rate
 * stacking (apply_lfr) and subsample-feats.  Both work on the time-major tensor
 * float [n_rows][n_planes][n_frames][stride] of which n_cols <= stride columns are
 * live: the output of mp3g_fbank_execute or mp3g_mfcc_execute, or of any call of
 * the three sections above.  lengths: uint32 [n_rows][len_planes], len_planes 1
 * (one count per row, as for mp3g_cmvn_rows) or n_planes (one per plane: the
 * lengths_out of mp3g_select_frames_rows as they stand); below, n =
 * min(lengths[r][p], n_frames).  Both are out of place (out must not overlap in)
 * and never write a word at a column past the live output width.  Every device
 * call (*_rows: device pointers throughout) equals its host call bit for bit, is
 * one launch whose shape depends on no buffer's contents, asynchronous on
 * hip_stream, and allocates nothing; all offsets are formed in 64 bits.
 *
 * Deltas: Kaldi's DeltaFeatures (add-deltas --delta-order=O --delta-window=W), as
 * stated HERE: this statement, written without Kaldi's source at hand, is the
 * definition the project tests.  The scales, in float32: scales[0] = {1}; for i =
 * 1..O, cur has len(prev) + 2 W zeros, and for j = -W..W ascending, then k over
 * prev ascending, cur[j + k + offset] += (float)j * prev[k] -- a float32 product,
 * then a float32 add, not fused -- and then every entry is multiplied by
 * (float)(1.0 / (double)norm), norm = the sum of j^2.  Order 2 is therefore built
 * from the already rounded order-1 scales.  mp3g_delta_scales writes them, order 0
 * first, order i as 2 i W + 1 floats: (O + 1) + W O (O + 1) floats in all.
 * out: float [n_rows][n_planes][n_frames][stride_out], stride_out >= (O + 1) *
 * n_cols.  For t < n, block 0 (columns [0, n_cols)) is a bit copy of the input
 * frame: -0 and NaN payloads survive.  Block i >= 1, column c: y = +0.0f; for j =
 * -i W..i W ascending, a tap whose scale is exactly 0 is skipped (as Kaldi skips
 * it: 0 * Inf stays out), any other is y = fmaf(scale_i[j], x[clamp(t + j, 0,
 * n - 1)][c], y).  Every order clamps on the ORIGINAL frames: order 2 is not order
 * 1 applied twice, and the two differ at a row's edges.  Frames t >= n are +0 in
 * all (O + 1) * n_cols live columns.  O = 0 is a copy with zero padding.
 * stride < n_cols, stride_out < (O + 1) * n_cols, W = 0, len_planes neither 1 nor
 * n_planes, out == in, out overlapping in or a null pointer with work to do is
 * MP3G_ERR_INVALID_ARGUMENT; O > 4 or O * W > 32 is MP3G_ERR_UNSUPPORTED; all
 * before any device call.  No rows, planes, frames or columns is MP3G_OK with
 * nothing done.
 *
 * Frame context: parameters left, right <= 64 (above: MP3G_ERR_UNSUPPORTED), step
 * >= 1 and first.  n_out(n) = 0 if n <= first, else ceil((n - first) / step):
 * mp3g_stack_frames_count.  out: float [n_rows][n_planes][n_frames_out]
 * [stride_out], stride_out >= (left + right + 1) * n_cols.  With m = min(n_out(n),
 * n_frames_out), output frame j < m has the anchor t = first + j * step, and its
 * block k = 0..left + right, columns [k * n_cols, (k + 1) * n_cols), is a bit copy
 * of input frame clamp(t - left + k, 0, n - 1); frames m <= j < n_frames_out are
 * +0 in their live columns; lengths_out (uint32 [n_rows][n_planes]) = m, written
 * whenever there is a row and a plane.
 *   splice-feats --left-context=L --right-context=R: left L, right R, step 1, first 0
 *   FunASR apply_lfr(m, n): left (m - 1) / 2, right m - 1 - left, step n, first 0
 *     (its left padding with frame 0, ceil(T / n) outputs, the last frame repeated)
 *   subsample-feats --n=N --offset=o: left 0, right 0, step N, first o
 * stride < n_cols, stride_out below the live width, step = 0, len_planes neither
 * 1 nor n_planes, out == in, out overlapping in or a null pointer with work to do
 * is MP3G_ERR_INVALID_ARGUMENT before any device call. */
int mp3g_delta_scales(uint32_t order, uint32_t window, float* out);
int mp3g_add_deltas_rows(int device, const float* d_in, float* d_out, uint32_t n_rows, uint32_t n_planes,
                         uint32_t n_frames, uint32_t stride, uint32_t n_cols, uint32_t stride_out,
                         const uint32_t* d_lengths, uint32_t len_planes, uint32_t order, uint32_t window,
                         void* hip_stream);
int mp3g_add_deltas_host(const float* in, float* out, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
                         uint32_t stride, uint32_t n_cols, uint32_t stride_out, const uint32_t* lengths,
                         uint32_t len_planes, uint32_t order, uint32_t window);
uint32_t mp3g_stack_frames_count(uint32_t n_frames, uint32_t step, uint32_t first);
int mp3g_stack_frames_rows(int device, const float* d_in, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames,
                           uint32_t stride, uint32_t n_cols, const uint32_t* d_lengths, uint32_t len_planes,
                           uint32_t left, uint32_t right, uint32_t step, uint32_t first, float* d_out,
                           uint32_t n_frames_out, uint32_t stride_out, uint32_t* d_lengths_out, void* hip_stream);
int mp3g_stack_frames_host(const float* in, uint32_t n_rows, uint32_t n_planes, uint32_t n_frames, uint32_t stride,
                           uint32_t n_cols, const uint32_t* lengths, uint32_t len_planes, uint32_t left,
                           uint32_t right, uint32_t step, uint32_t first, float* out, uint32_t n_frames_out,
                           uint32_t stride_out, uint32_t* lengths_out);

/* ---- Integrated loudness of decoded rows ----------------------------------------
 * ITU-R BS.1770-4 integrated loudness (what libebur128, pyloudnorm and ffmpeg's
 * loudnorm report as "I") and the sample peak of every row of a batch
 * float [n_rows][n_planes][T], n_planes 1 or 2, and a gain stage that brings the
 * rows to a target.  Both planes have channel weight 1; a mono row is one
 * channel.  The momentary and short-term maxima, the loudness range and the
 * true peak are the two sections below.  NOT offered: surround channel weights,
 * the momentary and short-term loudness as time series.
 *
 * mp3g_loudness_create(device, rate): rate 8000 .. 192000 (outside:
 * MP3G_ERR_UNSUPPORTED; rate <= 0 or a null pointer: MP3G_ERR_INVALID_ARGUMENT;
 * both with *out = NULL before any device call); device = -1 makes a host-only
 * object.  The K-weighting is two biquads designed in float64 from the analog
 * prototypes, as libebur128 and pyloudnorm design them (a0 = 1):
 *   shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196
 *     K = tan(pi f0 / rate), Vh = 10^(G/20), Vb = Vh^0.4996667741545416,
 *     a0 = 1 + K/Q + K^2;  b = [Vh + Vb K/Q + K^2, 2 (K^2 - Vh), Vh - Vb K/Q + K^2] / a0
 *     a = [1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0]
 *   high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, K and a0 alike;
 *     b = [1, -2, 1] (not normalised), a as above
 * (at 48 kHz the standard's printed table).  H = (rate + 5) / 10 in integers is
 * the 100 ms segment; a block is 4 H samples, the step H.  The filter state is
 * four doubles: the shelf's two, then the high-pass's two, transposed direct
 * form II.  From the filter code itself run on zero input from each unit state
 * e_k: V[n][k] the output at sample n < H, AH[m][k] the state after H samples,
 * G[a][b] = sum_n V[n][a] V[n][b] (n ascending); all float64, [k] fastest.
 *
 * The measurement.  len_r = T, or min(lengths[r], T) with lengths;
 * nseg = len_r / H, n_blocks = nseg >= 4 ? nseg - 3 : 0; samples past nseg H
 * take part only in the peak.  Everything below is float64 in the operation
 * order of go-mp3_amd/csrc/loudness_filter.h, without contraction.
 *   per (row, plane, segment j < nseg), from ZERO state, n ascending over its H
 *   samples: w[n] the K-weighted sample;  Ezs += w w;  g[k] += V[n][k] w;
 *   send = the state after the segment
 *   per (row, plane), j ascending, s0 = 0:
 *     E_j = max((Ezs_j + 2 (g_j . s0)) + s0^T G s0, 0);   s0 = AH s0 + send_j
 *   -- by superposition the sequential filter's segment energies, up to rounding
 *   per row: z_i = (sum over planes of ((E_i + E_i+1) + E_i+2) + E_i+3) / (4 H)
 *     absolute gate: z_i >= Ga = MP3G_LOUDNESS_ABS_GATE (-70 LUFS);
 *     relative gate: Gr = 0.1 (sum of the z_i >= Ga / n_abs);  a block counts when
 *     z_i >= Ga and z_i >= Gr;  energy = sum of those z_i / n_gated (i ascending)
 *     lufs = -0.691f + 10.0f * mp3g_log10f((float)energy); no gated block:
 *     energy = 0 and lufs = -inf
 *     peak = max |x[n]| over n < len_r and all planes: the sample peak
 * One record per row, mp3g_loudness_stats (32 bytes).  mp3g_loudness_host runs
 * exactly this decomposition, not a sequential filter, and mp3g_loudness_rows
 * equals it byte for byte.
 *
 * mp3g_loudness_rows: d_src, d_lengths (uint32 [n_rows], may be NULL), d_row_index
 * (uint32 [n_index] rows to measure, may be NULL: all n_rows; values >= n_rows
 * are skipped), d_scratch (mp3g_loudness_scratch_bytes, 8-byte aligned) and
 * d_stats ([n_rows] records) are device pointers.  Two launches whose shapes
 * depend on no device content, no allocation, asynchronous on hip_stream and
 * graph-capturable; writes the records of the rows it was given and its
 * scratch, nothing else.  A batch of mixed source rates is measured by one call
 * per rate through d_row_index.
 *
 * The gain stage, in place: per row g = (float)sqrt(target_energy / energy) (a
 * double division and square root, rounded once); with peak_ceiling > 0 and
 * peak > 0, g = min(g, peak_ceiling / peak) (a float32 division); energy == 0:
 * g = 1 and the row is not touched.  y[n] = x[n] * g for n < len_r, nothing else
 * is written; gain_out[r] = g when the pointer is given.  target_energy =
 * mp3g_loudness_target_energy(lufs) = 10^((lufs + 0.691) / 10), on the host.
 * mp3g_gain_rows equals mp3g_gain_host bit for bit; one launch. */
#define MP3G_LOUDNESS_ABS_GATE 1.1724653045822964e-07 /* the double nearest 10^-6.9309 */
typedef struct mp3g_loudness mp3g_loudness;
typedef struct mp3g_loudness_stats {
  double energy;      /* mean gated block energy; 0: no gated block */
  float lufs, peak;
  uint32_t n_blocks, n_abs, n_gated; /* blocks; past the absolute gate; past both */
  uint32_t zero;
} mp3g_loudness_stats;
int mp3g_loudness_create(int device, int rate, mp3g_loudness** out);
void mp3g_loudness_free(mp3g_loudness* ld);
/* H and views of the tables (valid while the object lives): shelf and highpass
 * as b0 b1 b2 a1 a2, V [H][4], AH [4][4], G [4][4].  Any pointer may be NULL. */
int mp3g_loudness_info(const mp3g_loudness* ld, uint32_t* H, const double** shelf, const double** highpass,
                       const double** V, const double** AH, const double** G);
uint64_t mp3g_loudness_blocks(const mp3g_loudness* ld, uint64_t n_samples);
int mp3g_loudness_host(const mp3g_loudness* ld, const float* x, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                       const uint32_t* lengths, mp3g_loudness_stats* stats);
uint64_t mp3g_loudness_scratch_bytes(const mp3g_loudness* ld, uint32_t n_rows, uint32_t n_planes, uint32_t T);
int mp3g_loudness_rows(const mp3g_loudness* ld, const float* d_src, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                       const uint32_t* d_lengths, const uint32_t* d_row_index, uint32_t n_index, void* d_scratch,
                       mp3g_loudness_stats* d_stats, void* hip_stream);
double mp3g_loudness_target_energy(double lufs);
int mp3g_gain_rows(int device, float* d_x, uint32_t n_rows, uint32_t n_planes, uint32_t T, const uint32_t* d_lengths,
                   const mp3g_loudness_stats* d_stats, double target_energy, float peak_ceiling, float* d_gain_out,
                   void* hip_stream);
int mp3g_gain_host(float* x, uint32_t n_rows, uint32_t n_planes, uint32_t T, const uint32_t* lengths,
                   const mp3g_loudness_stats* stats, double target_energy, float peak_ceiling, float* gain_out);

/* ---- True peak of decoded rows ---------------------------------------------------
 * The peak of the 4x oversampled signal (dBTP = 20 log10 of it), what
 * ebur128_true_peak and ffmpeg's ebur128 peak=true report, of every row of a
 * batch float [n_rows][n_planes][T], n_planes 1 or 2.  The interpolator is
 * libebur128's: 49 taps at factor 4, a Hann-windowed sinc designed in float64,
 *   j = 0..48, m = j - 24
 *   c[j] = (m == 0 ? 1 : sin(m pi/4) / (m pi/4)) * 0.5 (1 - cos(2 pi j / 48))
 * taps with |c[j]| <= 1e-6 dropped, phase f = j % 4, delay t = j / 4.  Phase 0 is
 * the single tap c[24] = 1 at delay 6: the sample itself.  Phases 1..3 have 12
 * taps each (t = 0..11), every one rounded once to float32
 * (go-mp3_amd/csrc/truepeak_coefs.inc from tools/gen_truepeak.py);
 * mp3g_true_peak_coefs gives them as [3][12].  Factor 4 is used at every rate:
 * MP3's rates end at 48 kHz, where libebur128 uses 4 as well (it takes 2 only
 * from 96 kHz on).
 *
 * The measurement, float32 with explicit fmaf and no other contraction
 * (go-mp3_amd/csrc/truepeak.h).  len_r = T, or min(lengths[r], T) with lengths.
 * Per plane and n < len_r, with x[k] = 0 for k < 0, for f = 1, 2, 3:
 *   y_f[n] = fmaf(c_f[11], x[n-11], ... fmaf(c_f[1], x[n-1], fmaf(c_f[0], x[n], 0)))
 * (the accumulator starts at 0, t ascends), and
 *   tp_r = max over planes, n and f of |y_f[n]|, and of |x[n]|,
 * updated as v > tp ? v : tp from tp = 0.  There is no tail flush: the ringing
 * after len_r is not evaluated (libebur128 does not evaluate it either).  Samples
 * at or past len_r and anything before a plane's first sample are never used.
 * The maximum is exact and order-free, so mp3g_true_peak_rows equals
 * mp3g_true_peak_host bit for bit.
 *
 * mp3g_true_peak_rows: d_src, d_lengths (uint32 [n_rows], may be NULL),
 * d_row_index (uint32 [n_index] rows to measure, may be NULL: all n_rows; values
 * >= n_rows are skipped), d_scratch (mp3g_true_peak_scratch_bytes, 4-byte
 * aligned; may be NULL when that is 0) and d_tp (float [n_rows]) are device
 * pointers.  Two launches whose shapes depend on no device content, no
 * allocation, asynchronous on hip_stream and graph-capturable; writes the d_tp
 * entries of the rows it was given and its scratch, nothing else.
 * mp3g_true_peak_tile: the samples of a plane one workgroup takes. */
int mp3g_true_peak_coefs(const float** c /* [3][12], phases 1..3 */);
uint32_t mp3g_true_peak_tile(void);
uint64_t mp3g_true_peak_scratch_bytes(uint32_t n_rows, uint32_t n_planes, uint32_t T);
int mp3g_true_peak_host(const float* x, uint32_t n_rows, uint32_t n_planes, uint32_t T, const uint32_t* lengths,
                        float* tp);
int mp3g_true_peak_rows(int device, const float* d_src, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                        const uint32_t* d_lengths, const uint32_t* d_row_index, uint32_t n_index, void* d_scratch,
                        float* d_tp, void* hip_stream);

/* ---- Momentary and short-term maxima, loudness range ---------------------------------
 * The rest of what EBU R128 meters and ffmpeg's loudnorm measure, from numbers
 * the loudness measure above has already formed: the largest momentary (400 ms)
 * and short-term (3 s) loudness of a row and its loudness range (EBU Tech 3342).
 *
 * The scratch of mp3g_loudness_rows, which this section reads.  With
 * S1 = T / H + 1 and n_work = n_index with d_row_index, else n_rows, it holds
 * n_work * n_planes * S1 items of 9 doubles, item ((i * n_planes + p) * S1 + j)
 * for work row i (row d_row_index[i], or i), plane p, segment j, then one float
 * per item.  After the call, for j < nseg: double 0 is the scanned segment
 * energy E^p_j, doubles 1..4 the segment pass's g and doubles 5..8 its send,
 * except that double 1 of plane 0's item i < n_blocks is the momentary block
 * energy z_i; the floats are the items' sample peaks (item nseg: the ragged
 * tail's).
 *
 * Everything below is float64 in the operation order of
 * go-mp3_amd/csrc/loudness_range.h, without contraction; nseg, n_blocks, H and
 * Ga = MP3G_LOUDNESS_ABS_GATE as above.
 *   momentary: M = max_i z_i;  momentary_max = M > 0 ?
 *     -0.691f + 10.0f * mp3g_log10f((float)M) : -inf
 *   short-term: n_short = nseg >= 30 ? nseg - 29 : 0;
 *     P^p_k = (((E^p_k + E^p_k+1) + ...) + E^p_k+29);  S_k = (P^0_k [+ P^1_k]) / (30 H)
 *     -- a 3 s block every segment (100 ms, ffmpeg's step; Tech 3342 asks for 1 s
 *     or less);  shortterm_max from max_k S_k as momentary_max from M
 *   range: absolute gate S_k >= Ga, sum_abs and n_abs over k ascending;
 *     relative gate rel = 0.01 * (sum_abs / n_abs) (-20 LU);  the gated set is
 *     S_k >= Ga && S_k >= rel, n_range its count;  among the gated values in
 *     ascending order lo has rank ((n_range - 1) * 10 + 50) / 100 and hi rank
 *     ((n_range - 1) * 95 + 50) / 100 (integer division: the nearest rank, as
 *     libebur128 and the Tech 3342 reference take it);  range_lo and range_hi
 *     are -0.691f + 10.0f * mp3g_log10f((float)v), lra = range_hi - range_lo in
 *     float32;  n_range == 0: lra = 0, range_lo = range_hi = -inf
 * The selected values do not depend on how ties are ordered.  One record per
 * row, mp3g_loudness_range (32 bytes).
 *
 * mp3g_loudness_range_host runs mp3g_loudness_host's segment pass, scan and
 * blocks and then the above.  mp3g_loudness_range_rows reads d_loudness_scratch
 * -- the scratch EXACTLY as mp3g_loudness_rows left it when called with the same
 * object and the same n_rows, n_planes, T, d_lengths, d_row_index and n_index
 * earlier on the same stream -- and writes d_range_scratch
 * (mp3g_loudness_range_scratch_bytes, 8-byte aligned) and the records of the
 * rows it was given, nothing else; it equals the host byte for byte.  One launch
 * whose shape depends on no device content, no allocation, asynchronous on
 * hip_stream and graph-capturable. */
typedef struct mp3g_loudness_range {
  float momentary_max, shortterm_max; /* LUFS; -inf: no block */
  float lra, range_lo, range_hi;      /* LU, LUFS, LUFS */
  uint32_t n_short, n_range;          /* short-term blocks; past both gates */
  uint32_t zero;
} mp3g_loudness_range;
int mp3g_loudness_range_host(const mp3g_loudness* ld, const float* x, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                             const uint32_t* lengths, mp3g_loudness_range* out);
uint64_t mp3g_loudness_range_scratch_bytes(const mp3g_loudness* ld, uint32_t n_rows, uint32_t n_planes, uint32_t T);
int mp3g_loudness_range_rows(const mp3g_loudness* ld, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                             const uint32_t* d_lengths, const uint32_t* d_row_index, uint32_t n_index,
                             const void* d_loudness_scratch, void* d_range_scratch, mp3g_loudness_range* d_out,
                             void* hip_stream);

/* The gain stage against a supplied peak: mp3g_gain_rows and mp3g_gain_host with
 * peak[r] (float [n_rows]; a true peak, say) in place of the records' sample
 * peak.  With the pointer NULL they are mp3g_gain_rows and mp3g_gain_host, bit
 * for bit. */
int mp3g_gain_rows_peak(int device, float* d_x, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                        const uint32_t* d_lengths, const mp3g_loudness_stats* d_stats, double target_energy,
                        float peak_ceiling, float* d_gain_out, void* hip_stream, const float* d_peak);
int mp3g_gain_host_peak(float* x, uint32_t n_rows, uint32_t n_planes, uint32_t T, const uint32_t* lengths,
                        const mp3g_loudness_stats* stats, double target_energy, float peak_ceiling, float* gain_out,
                        const float* peak);

/* ---- Room reverberation and noise at an SNR -------------------------------------
 * The augmentation Kaldi's x-vector recipes train on (wav-reverberate is the
 * model): a batch float [n_rows][n_planes][T], n_planes 1 or 2, is convolved row
 * by row with a room impulse response (RIR), has noises added at signal-to-noise
 * ratios measured against the EARLY reverberation, and is brought back to its
 * power.  Every plane of a row gets the row's RIR and noises; every power is per
 * (row, plane).  n = min(lengths[r], T) below (lengths NULL: T).  Deliberately
 * unlike the tool: only the shifted output of the input's length, a noise's
 * start counted on the output's timeline, powers per plane.  NOT offered: speed
 * and volume perturbation, multi-channel RIRs, an output length that depends on
 * the data.
 *
 * The sums.  Every power is a float64 sum of exact products (double)a *
 * (double)a in ONE order: the samples are cut into blocks of 1,024, a block's
 * products are added ascending from +0.0, then the block sums ascending from
 * +0.0; power = sum / count, an IEEE float64 division (count 0: +0.0).  The
 * blocks of x, of a noise row and of the mixed signal start at the row's sample
 * 0; those of the early reverberation are the blocks [1024 k, 1024 k + 1024) of
 * the full convolution's timeline, cut to [es, n + ee - 1).
 * mp3g_row_power_rows / _host: power[r] = that of x[r][0 .. min(lengths[r], T))
 * for float [n_rows][T] -- the noise bank's Pn.  Two launches, d_scratch of
 * mp3g_row_power_scratch_bytes (8-byte aligned).
 *
 * mp3g_reverb_create(device, rate, rirs, n_rirs, stride, rir_lengths): a bank of
 * n_rirs >= 1 responses, host float [n_rirs][stride], response i of L =
 * rir_lengths[i] taps, 1 <= L <= 65,536 and L <= stride (else
 * MP3G_ERR_INVALID_ARGUMENT), rate 20 .. 384000 (outside: MP3G_ERR_UNSUPPORTED;
 * rate <= 0: MP3G_ERR_INVALID_ARGUMENT; below 20 Hz the early window would be
 * empty); device = -1 makes a host-only object.  Per response h:
 *   peak = the first index of the largest VALUE (not magnitude; h[j] > h[peak],
 *          j ascending)
 *   es = max(0, peak - rate / 1000),  ee = min(L, peak + rate / 20)  (integer
 *        divisions: the truncations of 0.001 rate and 0.05 rate)
 *   h_e = h on [es, ee), 0 elsewhere: the early response
 *   P = ceil(L / 1024) partitions;  G_p = FFT_2048 of g_p[j] = h[1024 p + j] +
 *       i h_e[1024 p + j] for j < 1024 (0 past L), 0 for j >= 1024
 * The transform is go-mp3_amd/csrc/reverb_fft.h's: the STFT's float32
 * decimation-in-frequency network (2,048 complex points, twiddles exp(-2 pi i k /
 * 4096) from float64, rounded once), bins left in slot order.  mp3g_reverb_info:
 * the table [n_rirs][8] words L, peak, es, ee, P, 0 and the 64-bit offset of G_0
 * in the spectra (complex values), the twiddles [4096][2], the spectra
 * [n_spectra][2]; any pointer may be NULL.  mp3g_reverb_read_spectra copies the
 * DEVICE's spectra to host (synchronous; for tests).
 *
 * mp3g_augment_args.  x, out, lengths (may be NULL), rir_index (int32 [n_rows],
 * may be NULL: no row has a response; < 0: this row has none), noise (float
 * [n_noise][Tn]), noise_lengths (uint32 [n_noise], clamped to Tn), noise_power
 * (double [n_noise], mp3g_row_power_*), slots (mp3g_augment_slot [n_rows][A], A
 * <= 8) and stats (double [n_rows][n_planes][4]) are host pointers for
 * mp3g_augment_host and device pointers for mp3g_augment_rows, which takes host
 * copies of rir_index, noise_lengths and slots beside them for its checks.  A
 * slot: noise_index (< 0: none), snr_ratio = 10^(-snr_dB / 10) formed by the
 * caller in float64 (no pow runs on the device), start in output samples,
 * offset < the noise's length, wrap (non-zero: the noise repeats cyclically to
 * the row's end; zero: it adds min(len - offset, n - start) samples).
 *
 * Per (row, plane):
 *   1 power_before = power of x[0 .. n)
 *   2 with a response: y[o] = (x * h)[o + peak], 0 <= o < n (the tool's
 *     --shift-output=true);  signal_power = sum over t in [es, n + ee - 1) of
 *     (x * h_e)[t]^2 / (n + (ee - es) - 1).  Without: y = x as bits and
 *     signal_power = power_before.
 *     The convolutions, float32 in one order: with NB = ceil(n / 1024), X_m =
 *     FFT_2048 of (x[1024 (m - 1) + j], 0), j < 2048, 0 <= m <= NB (x = 0 outside
 *     [0, n)); for output block k in [es / 1024, (n + ee - 2) / 1024]:
 *       acc = (+0, +0);  for p ascending, max(0, k - NB) <= p <= min(P - 1, k):
 *         acc += X_(k-p) G_p slot by slot, a product (a + i b)(c + i d) as t = b d,
 *         re = fmaf(a, c, -t), u = b c, im = fmaf(a, d, u), then one float32
 *         addition per part
 *       z = the transposed (decimation-in-time) network of reverb_fft.h on acc,
 *       conjugated twiddles, slot order in, natural order out;  for j < 1024, t =
 *       1024 k + j:  (x * h)[t] = z[1024 + j].re * 2^-11,  (x * h_e)[t] = z[1024 +
 *       j].im * 2^-11
 *   3 v = y;  for the slots in ascending order, skipping noise_index < 0 and Pn ==
 *     0:  g = (float)sqrt(snr_ratio * signal_power / Pn) (the product first; IEEE
 *     float64), and for start <= j < n with the slot's noise sample at offset + (j -
 *     start) (modulo len with wrap; none past len without): v[j] = fmaf(g, noise, v[j])
 *   4 power_after = power of v[0 .. n);  with MP3G_AUGMENT_NORMALIZE: scale =
 *     sqrt(power_before / power_after), 1.0 where power_after == 0 or n == 0, and
 *     out[j] = (float)((double)v[j] * scale); without: scale = 1.0 and out = v as
 *     bits.  out[j] = +0 for n <= j < T.
 *   stats = power_before, signal_power, power_after, scale.
 * out is out of place: overlapping x is MP3G_ERR_INVALID_ARGUMENT, as are A > 8,
 * an unknown flag, rir_index >= n_rirs (or >= 0 without an object), noise_index
 * >= n_noise, offset >= the noise's length and a null buffer with work to do;
 * all before any device call.  No rows or T == 0 is MP3G_OK with nothing done.
 *
 * mp3g_augment_rows equals mp3g_augment_host bit for bit, out and stats.  Five
 * launches whose shapes depend on n_rows, n_planes, T and the object's longest
 * response only, no atomics, no allocation, asynchronous on hip_stream and
 * graph-capturable; d_scratch of at least mp3g_reverb_scratch_bytes(rv, ...)
 * bytes (8-byte aligned; rv may be NULL for a call without responses), a smaller
 * scratch_bytes or a NULL scratch is MP3G_ERR_INVALID_ARGUMENT. */
#define MP3G_AUGMENT_NORMALIZE 1u
typedef struct mp3g_reverb mp3g_reverb;
typedef struct mp3g_augment_slot {
  int32_t noise_index;
  uint32_t start, offset, wrap;
  double snr_ratio;
} mp3g_augment_slot; /* 24 bytes */
typedef struct mp3g_augment_args {
  const float* x;
  float* out;
  const uint32_t* lengths;
  const int32_t* rir_index;
  const float* noise;
  const uint32_t* noise_lengths;
  const double* noise_power;
  const mp3g_augment_slot* slots;
  double* stats;
  uint32_t n_rows, n_planes, T, n_noise, Tn, A, flags, zero;
} mp3g_augment_args;
int mp3g_reverb_create(int device, int rate, const float* rirs, uint32_t n_rirs, uint32_t stride,
                       const uint32_t* rir_lengths, mp3g_reverb** out);
void mp3g_reverb_free(mp3g_reverb* rv);
int mp3g_reverb_info(const mp3g_reverb* rv, uint32_t* n_rirs, uint32_t* max_taps, const uint32_t** table,
                     const float** twiddles, const float** spectra, uint64_t* n_spectra);
int mp3g_reverb_read_spectra(const mp3g_reverb* rv, float* spectra);
uint64_t mp3g_reverb_scratch_bytes(const mp3g_reverb* rv, uint32_t n_rows, uint32_t n_planes, uint32_t T);
int mp3g_augment_host(const mp3g_reverb* rv, const mp3g_augment_args* args);
int mp3g_augment_rows(const mp3g_reverb* rv, int device, const mp3g_augment_args* d_args, const int32_t* rir_index,
                      const uint32_t* noise_lengths, const mp3g_augment_slot* slots, void* d_scratch,
                      uint64_t scratch_bytes, void* hip_stream);
uint64_t mp3g_row_power_scratch_bytes(uint32_t n_rows, uint32_t T);
int mp3g_row_power_host(const float* x, uint32_t n_rows, uint32_t T, const uint32_t* lengths, double* power);
int mp3g_row_power_rows(int device, const float* d_x, uint32_t n_rows, uint32_t T, const uint32_t* d_lengths,
                        void* d_scratch, double* d_power, void* hip_stream);

/* ---- STFT and mel spectrograms of decoded rows --------------------------------
 * The front ends of music and general audio at its native rate: an STFT by FFT
 * for n_fft = P in {256, 512, 1024, 2048, 4096}, stored as complex bins, power
 * or magnitude, with an optional mel filter bank (Slaney's or HTK's scale, with
 * or without area normalisation) and an optional logarithm.  Every value is a
 * fixed sequence of float32 operations, so the device call equals
 * mp3g_stft_host bit for bit.  No reference counterpart.
 *
 * Parameters.  rate > 0; 1 <= win_length <= P; 1 <= hop <= P; output one of
 * MP3G_STFT_COMPLEX / _POWER / _MAGNITUDE; n_mels in 0..128 (0: no mel bank,
 * the K = P / 2 + 1 bins are the output); fmin, fmax as mp3g_logmel_create takes
 * them; log one of MP3G_STFT_LOG_NONE / _LN / _LOG10; floor a normal positive
 * float32 when log != NONE (ignored otherwise); flags MP3G_STFT_CENTER,
 * MP3G_STFT_MEL_HTK, MP3G_STFT_MEL_NORM.  MP3G_STFT_COMPLEX with n_mels > 0 or a
 * logarithm is MP3G_ERR_INVALID_ARGUMENT; an n_fft that is none of the five
 * sizes or an n_mels outside 0..128 MP3G_ERR_UNSUPPORTED; every other bad value
 * MP3G_ERR_INVALID_ARGUMENT; all before any device call, with *out = NULL.
 *
 * Framing is mp3g_logmel's: with MP3G_STFT_CENTER pad = P / 2, frame f reads
 * xr[f hop - pad + n], n < P, xr the row reflected about both ends, T > pad,
 * frames 0 .. T / hop; without it pad = 0 and the frames are 0 .. (T - P) / hop.
 *
 * Tables, computed in float64 and rounded once to float32:
 *   w[n], n < P: the periodic Hann window of win_length centred in the frame
 *     (torch.stft): L = (P - win_length) / 2, w[L + j] = 0.5 - 0.5 cos(2 pi j /
 *     win_length) for j < win_length, 0 elsewhere; win_length = 1: w[L] = 1.
 *   tw[k] = (cos(2 pi k / P), -sin(2 pi k / P)), k < P; k a multiple of P / 4 is
 *     exactly (1, 0), (0, -1), (-1, 0), (0, 1).
 *   Wm[m][k]: triangles in Hz between n_mels + 2 points equally spaced on the
 *     mel scale (Slaney's as in mp3g_logmel; MP3G_STFT_MEL_HTK: 2595 log10(1 +
 *     f / 700)), as librosa.filters.mel and torchaudio's melscale_fbanks build
 *     them; MP3G_STFT_MEL_NORM scales filter m by 2 / (its width in Hz).
 *
 * Features, all float32; the order is part of the contract:
 *   v[n] = w[n] * xr[f hop - pad + n]                     (one rounded product)
 *   z[n] = v[2 n] + i v[2 n + 1], n < N = P / 2
 *   Z = FFT_N(z): decimation in frequency, in place; radix-4 passes over blocks
 *     of len = N, N / 4, .. >= 4, then a radix-2 pass if len = 2 is left.  The
 *     radix-4 butterfly at block base b, n < q = len / 4, x_r = z[b + n + r q]:
 *       t0 = x0 + x2, t1 = x0 - x2, t2 = x1 + x3, t3 = -i (x1 - x3)
 *       z[b+n] = t0 + t2,            z[b+n+q]  = (t1 + t3) tw[n P / len],
 *       z[b+n+2q] = (t0 - t2) tw[2 n P / len], z[b+n+3q] = (t1 - t3) tw[3 n P / len]
 *     (radix 2: x0 + x1, x0 - x1).  A product (a + i b)(c + i d), c + i d the
 *     table entry, is t = b * d, re = fmaf(a, c, -t), u = b * c, im = fmaf(a, d,
 *     u); with a table index that is a multiple of P / 4 it is a move with
 *     negations.  Z[k] stands where k's digits (base 4 from the low end, then
 *     the last bit) are reversed.
 *   E = (Z[k].re + Z[N-k].re, Z[k].im - Z[N-k].im), O = (Z[k].re - Z[N-k].re,
 *   Z[k].im + Z[N-k].im), T = O tw[k], for 0 < k <= N / 2:
 *     X[k]   = ((E.re + T.im) * 0.5f, (E.im - T.re) * 0.5f)
 *     X[N-k] = ((E.re - T.im) * 0.5f, (-E.im - T.re) * 0.5f)
 *   (bin N / 2 is X[k]'s formula at k = N / 2: the two differ in a zero's sign)
 *   X[0] = (Z[0].re + Z[0].im, +0), X[N] = (Z[0].re - Z[0].im, +0)
 *   -- torch.stft's sign; a frame's bits depend on its own P samples only.
 *   MP3G_STFT_COMPLEX stores (re, im); _POWER p = fmaf(re, re, im * im);
 *   _MAGNITUDE sqrtf(p), correctly rounded.
 *   n_mels > 0: mel = +0; for k = lo_m .. hi_m: mel = fmaf(Wm[m][k], s[k], mel),
 *     s the power or the magnitude (empty filters allowed).
 *   log: y = mp3g_logf(max(s, floor)) or mp3g_log10f(max(s, floor)), the
 *     logarithms of the two feature objects above.  No clamp.
 *
 * Domain: finite samples with |x| <= 2^20; float32 subnormals are kept.
 * Output, frequency-major: float [row][plane][bins][frame_stride] with bins =
 * n_mels ? n_mels : K; MP3G_STFT_COMPLEX: float [row][plane][K][frame_stride][2]
 * (torch.view_as_real of torch.stft's [.., K, F]).  n_frames entries are
 * written per bin row, nothing else. */
#define MP3G_STFT_CENTER 1u
#define MP3G_STFT_MEL_HTK 2u
#define MP3G_STFT_MEL_NORM 4u
#define MP3G_STFT_COMPLEX 0
#define MP3G_STFT_POWER 1
#define MP3G_STFT_MAGNITUDE 2
#define MP3G_STFT_LOG_NONE 0
#define MP3G_STFT_LOG_LN 1
#define MP3G_STFT_LOG_LOG10 2
#define MP3G_STFT_MIN_FFT 256
#define MP3G_STFT_MAX_FFT 4096
#define MP3G_STFT_MAX_MELS 128
typedef struct mp3g_stft mp3g_stft;
/* Builds the tables; device >= 0 also uploads them to that device (once),
 * device = -1 makes a host-only object. */
int mp3g_stft_create(int device, int rate, int n_fft, int win_length, int hop, int output, int n_mels, double fmin,
                     double fmax, int log, float floor, uint32_t flags, mp3g_stft** out);
void mp3g_stft_free(mp3g_stft* st);
/* K, the window float [n_fft], the twiddles float [n_fft][2], Wm float
 * [n_mels][K] and the supports uint32 [n_mels][2] = lo_m, hi_m (lo > hi: an
 * empty filter; both NULL without a mel bank) -- all owned by the object -- and
 * the frames a workgroup of the device call produces (any may be NULL). */
int mp3g_stft_info(const mp3g_stft* st, uint32_t* K, const float** window, const float** twiddles, const float** wm,
                   const uint32_t** support, uint32_t* tile_frames);
/* The frames a row of T samples has (0: none, or T >= 2^62). */
uint64_t mp3g_stft_frames(const mp3g_stft* st, uint64_t T);
/* The definition above in plain C++ (the reference the device call equals):
 * out[b * frame_stride + f] (MP3G_STFT_COMPLEX: out[(b * frame_stride + f) * 2
 * + 0 / 1]) for b < bins, f < n_frames <= mp3g_stft_frames. */
int mp3g_stft_host(const mp3g_stft* st, const float* x, uint64_t T, uint64_t n_frames, float* out,
                   uint64_t frame_stride);
/* d_src: float [n_rows][n_planes][T]; d_out as above.  Both are device pointers
 * and the launch shape depends on none of their contents: one launch,
 * asynchronous on hip_stream and graph-capturable; launches of one object need
 * no ordering between them.  T < 2^31; n_frames <= mp3g_stft_frames(st, T),
 * frame_stride >= n_frames. */
int mp3g_stft_execute(const mp3g_stft* st, const float* d_src, uint32_t n_rows, uint32_t n_planes, uint32_t T,
                      float* d_out, uint32_t n_frames, uint32_t frame_stride, void* hip_stream);

/* ---- decoder: mp3.NewDecoder / io.Reader / io.Seeker (decode.go:27-388) ----
 * Scans on the host with read-ahead (headers, side info, reservoir) and
 * decodes batches of frames on `device`: scale factors + Huffman codes with
 * the main-data kernel, then the DSP (mode = MP3G_MODE_EXACT | MP3G_MODE_FAST,
 * | MP3G_FLAG_HOST_HUFFMAN for the host parse instead of the Huffman kernel).  `data` is copied.
 * seekable = 0 models a reader that is not an io.Seeker (Length = -1).
 * Read returns MP3G_OK with *n >= 1, MP3G_EOF, or the error of the frame
 * that failed (after all PCM before it was delivered) -- like Decoder.Read. */
typedef struct mp3g_decoder mp3g_decoder;
int mp3g_decoder_new(const uint8_t* data, size_t len, int seekable, int device, uint32_t mode,
                     mp3g_decoder** out);

/* Streaming input: the caller's io.Reader (and io.Seeker) as callbacks, so a
 * decoder runs on input it has not got yet -- a pipe, a socket, a live radio
 * stream -- and pulls bytes as it needs them, like the reference's source
 * (source.go:99-122, io.ReadFull on the reader).  mp3.NewDecoder(r)
 * (decode.go:361-388) is mp3g_decoder_new_reader: it returns once the tags
 * and frame 0 are in (for a seeker, after the header walk of
 * ensureFrameStartsAndLength, decode.go:154-216, as the reference does).
 *   read : io.Reader.Read -- write up to `cap` bytes to `buf`, return the
 *          count; 0 = io.EOF; < 0 = an error (the decoder call in progress
 *          returns MP3G_ERR_READ; a later call asks the reader again).
 *   seek : io.Seeker.Seek (whence 0/1/2), the new offset or < 0 on error; NULL
 *          when the reader is no io.Seeker (Length = -1, Seek fails as the
 *          reference's does, source.go:28-33).
 *   user : passed back to the callbacks verbatim, never dereferenced (for
 *          cgo: a runtime/cgo.Handle, not a Go pointer).
 * Read-ahead policy: with a seek callback (a file-like source) the decoder
 * reads ahead in batches; without one it calls `read` only when it holds no
 * complete frame it has not decoded -- exactly when the reference's
 * Decoder.Read blocks on its reader -- so every frame whose bytes have
 * arrived is delivered without waiting for more input.  The callbacks run on
 * the thread that calls into the decoder, only during that call. */
typedef struct mp3g_reader {
  int64_t (*read)(void* user, uint8_t* buf, size_t cap);
  int64_t (*seek)(void* user, int64_t offset, int whence);
  void* user;
} mp3g_reader;
int mp3g_decoder_new_reader(const mp3g_reader* reader, int device, uint32_t mode, mp3g_decoder** out);
void mp3g_decoder_free(mp3g_decoder* dec);
int mp3g_decoder_read(mp3g_decoder* dec, uint8_t* buf, size_t cap, size_t* n);
/* io.ReadFull over Decoder.Read (Go's io.ReadFull loops Read the same way):
 * repeated reads until `cap` bytes, EOF or an error.  Returns MP3G_OK with
 * *n == cap, or the status that ended it (MP3G_EOF / the frame's error) with
 * *n = the bytes delivered before it.  One call instead of one per frame. */
int mp3g_decoder_read_full(mp3g_decoder* dec, uint8_t* buf, size_t cap, size_t* n);
/* whence: 0 = io.SeekStart, 1 = io.SeekCurrent, 2 = io.SeekEnd */
int mp3g_decoder_seek(mp3g_decoder* dec, int64_t offset, int whence, int64_t* newpos);
/* SampleRate, Length (-1 if unknown), BytesPerFrame, current position (bytes) */
int mp3g_decoder_info(const mp3g_decoder* dec, int* sample_rate, int64_t* length, int64_t* bytes_per_frame,
                      int64_t* position);
/* time API; durations are time.Duration nanoseconds */
int64_t mp3g_decoder_duration_ns(const mp3g_decoder* dec);
int64_t mp3g_decoder_position_ns(const mp3g_decoder* dec);
int64_t mp3g_decoder_remaining_ns(const mp3g_decoder* dec);
double mp3g_decoder_progress(const mp3g_decoder* dec);
int64_t mp3g_decoder_sample_position(const mp3g_decoder* dec);
int64_t mp3g_decoder_sample_count(const mp3g_decoder* dec);
int mp3g_decoder_seek_to_sample(mp3g_decoder* dec, int64_t sample);
int mp3g_decoder_seek_to_time_ns(mp3g_decoder* dec, int64_t t_ns);
int mp3g_decoder_skip_ns(mp3g_decoder* dec, int64_t delta_ns);

/* ---- diagnostics (not part of the decode contract) -----------------------
 * Runs a FAST-mode plan once through the s_memtime-instrumented build of the
 * fast kernel and returns, per kernel phase, the shader cycles summed over
 * all chunks (out_cycles[0..7]: parameters, requantize, stereo+antialias,
 * IMDCT, S rows into the ring, matrixing (DCT-32), window+store, history
 * shift).  PCM is written as by mp3g_plan_execute.  Synchronous. */
int mp3g_plan_debug_phases(mp3g_plan* plan, const mp3g_granule* d_granules, const int16_t* d_coeffs,
                           int16_t* d_pcm, uint64_t* out_cycles, void* hip_stream);
/* The same instrumented launch; per chunk (out_ticks[4 * chunk + 0..3]) the
 * wave's s_memrealtime (100 MHz) at kernel entry, at the start and the end of
 * its granule loop and at exit: the launch's ramp, per-wave span and tail. */
int mp3g_plan_debug_timeline(mp3g_plan* plan, const mp3g_granule* d_granules, const int16_t* d_coeffs,
                             int16_t* d_pcm, uint64_t* out_ticks, void* hip_stream);

/* Shader clock under load: launches n_waves one-wave workgroups on
 * hip_stream that spin until the device word *d_flag turns non-zero (set it
 * from another stream after the work to be measured) or max_ms (<= 10,000)
 * pass, each writing 5 uint64 to d_out[5 * wg ..]: s_memtime (shader cycles)
 * and s_memrealtime (100 MHz) at the start and the end of its window, and
 * whether it saw the flag.  Asynchronous. */
int mp3g_debug_clock_probe(int device, const uint32_t* d_flag, uint64_t* d_out, uint32_t n_waves,
                           uint32_t max_ms, void* hip_stream);

/* One launch of mp3g_augment_rows, which = 0 .. 4 (the power of x, the forward
 * transforms, the convolution, the mix, the scale), with that call's arguments
 * and checks: for timing a launch on buffers a whole call has filled
 * (tools/reverb_time.py).  Run alone, the mix and the scale work on what `out`
 * holds, so the samples are no longer the contract's. */
int mp3g_augment_debug_launch(const mp3g_reverb* rv, int device, const mp3g_augment_args* d_args,
                              const int32_t* rir_index, const uint32_t* noise_lengths,
                              const mp3g_augment_slot* slots, void* d_scratch, uint64_t scratch_bytes,
                              void* hip_stream, uint32_t which);

/* ---- Xing / Info / LAME tag (lameinfo/lameinfo.go) ----
 * The reference's lameinfo package: the tag in the first frame (encoder delay
 * and padding for gapless playback, frame / byte counts, the VBR seek TOC).
 * The decoder never reads it (decode.go decodes the tag frame as silence);
 * callers trim with the two totals.  140 bytes. */
#define MP3G_XING_FRAME_COUNT 0x0001u /* lameinfo.FlagFrameCount */
#define MP3G_XING_BYTE_COUNT 0x0002u  /* FlagByteCount */
#define MP3G_XING_TOC 0x0004u         /* FlagTOC */
#define MP3G_XING_VBR_SCALE 0x0008u   /* FlagVBRScale */
#define MP3G_LAME_DECODER_DELAY 529   /* lameinfo.DecoderDelay */
typedef struct mp3g_lame_info {
  uint32_t is_xing;         /* Info.IsXing: tag "Xing" (VBR) vs "Info" (CBR) */
  uint32_t flags;           /* Info.Flags */
  uint32_t frame_count;     /* Info.FrameCount */
  uint32_t byte_count;      /* Info.ByteCount */
  uint8_t toc[100];         /* Info.TOC */
  uint32_t vbr_scale;       /* Info.VBRScale */
  uint32_t has_lame;        /* Info.HasLAMEInfo(): LAMEVersion != "" */
  char lame_version[12];    /* Info.LAMEVersion: the 9 bytes as stored (may hold NULs), zero padded */
  uint16_t encoder_delay;   /* Info.EncoderDelay */
  uint16_t encoder_padding; /* Info.EncoderPadding */
} mp3g_lame_info;

/* lameinfo.Parse (lameinfo.go:139-270): one whole frame incl. its header.
 * MP3G_OK or MP3G_ERR_NO_XING_HEADER. */
int mp3g_lame_parse(const uint8_t* frame, size_t len, mp3g_lame_info* out);
/* lameinfo.ParseFromReader (lameinfo.go:288-328) on a reader positioned at
 * `data`: reads the header, sizes the frame, reads the frame, parses it.
 * MP3G_OK, MP3G_ERR_NO_XING_HEADER, MP3G_EOF (io.EOF) or
 * MP3G_ERR_UNEXPECTED_EOF; *consumed (may be NULL) = bytes read. */
int mp3g_lame_parse_reader(const uint8_t* data, size_t len, mp3g_lame_info* out, size_t* consumed);
/* Info.TotalDelay / Info.TotalPadding (lameinfo.go:92-111) */
int mp3g_lame_total_delay(const mp3g_lame_info* info);
int mp3g_lame_total_padding(const mp3g_lame_info* info);
/* Gapless trim of n_samples decoded samples (per channel) of a stream whose
 * first frame held the tag: keep [*first, *first + *count); tag_frame_samples
 * = what the decoder produced for the tag frame (1152 MPEG-1, 576 MPEG-2).
 * The reference only exposes the two totals; this applies them. */
int mp3g_lame_trim(const mp3g_lame_info* info, uint64_t n_samples, uint32_t tag_frame_samples, uint64_t* first,
                   uint64_t* count);
/* Xing TOC seek: *offset = byte offset of `percent` (0..100) of the playback
 * time, from Info.TOC (lameinfo.go:33-35) scaled by the tag's byte count
 * (flag 0x2) or, when the tag carries none, by `stream_bytes` (the caller's
 * audio byte length); linear without a TOC.  MP3G_ERR_INVALID_ARGUMENT (and
 * *offset = 0) when neither byte count is known. */
int mp3g_lame_toc_offset(const mp3g_lame_info* info, double percent, uint64_t stream_bytes, uint64_t* offset);

#ifdef __cplusplus
}
#endif
#endif /* MP3G_H */
