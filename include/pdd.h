/*
 * pdd.h — C ABI of libpdd.so, the MI355X (gfx950) incoherent-dedispersion
 * engine behind pypulsar's `Spectra` hot path.
 *
 * Conventions:
 *   - every entry point returns int status: 0 = ok, < 0 = error;
 *     pdd_last_error() returns a thread-local message for the last failure;
 *   - all array pointers are DEVICE pointers owned by the caller (torch
 *     tensors or any hipMalloc'd memory) unless the name says `host_`;
 *     the library never frees caller memory;
 *   - every compute call takes a hipStream_t (passed as void*) and is
 *     asynchronous on it; pdd_sync() is the only synchronisation;
 *   - 2-D arrays are row-major with an explicit leading dimension `ld`
 *     (elements between consecutive rows);
 *   - the delay-bin tables are built on the host in float64 (bit-exact with
 *     the reference) and passed in as int32.
 *
 * Each entry point cites the reference interface it replaces (file:line in
 * emilieparent/pypulsar).
 */
#ifndef PDD_H
#define PDD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element types */
enum { PDD_F32 = 0, PDD_U8 = 1, PDD_U16 = 2 };
/* pad modes (Spectra.shift_channels padval, formats/spectra.py:81-94) */
enum {
  PDD_PAD_VALUE = 0,  /* per-channel pad value from `padvals` (number / 'mean' / 'median') */
  PDD_PAD_ROTATE = 1  /* psr_utils.rotate wrap-around (padval == 'rotate') */
};
/* channel statistics: pad values for 'mean'/'median' (spectra.py:83-86);
 * std (population, float64 two-pass), min, max for scaled/scaled2
 * (spectra.py:140-188) */
enum { PDD_STAT_MEAN = 0, PDD_STAT_MEDIAN = 1, PDD_STAT_STD = 2, PDD_STAT_MIN = 3, PDD_STAT_MAX = 4 };
/* zero-DM layouts */
enum { PDD_LAYOUT_TIME_MAJOR = 0, /* [nspec][nchan], filterbank file order */
       PDD_LAYOUT_CHAN_MAJOR = 1  /* [nchan][nspec], Spectra.data order    */ };

int pdd_version(void);
const char* pdd_last_error(void);
/* Identity of this build: the 16-hex-digit digest of the HIP sources and
 * compile flags the library was built from (pypulsar_amd/_digest.py computes
 * the same from a source tree).  The Python host refuses a library whose
 * digest differs from its sources, and profiling evidence is stamped with it,
 * so counters are only reported for the binary that produced them. */
const char* pdd_source_digest(void);
/* Free the device scratch the library keeps per (device, stream, calling host
 * thread) -- sweep images, partial sums; synchronises the device.  Optional:
 * the next call that needs scratch allocates it again.  Scratch is keyed by
 * the calling thread, so several host threads may queue work on one stream
 * (each gets its own buffers, e.g. an 8 GiB sweep image each); a thread's
 * buffers stay allocated after it exits until this call.  Returns the first
 * HIP error (every buffer is still freed). */
int pdd_scratch_release(void);
/* hipStreamSynchronize(stream) */
int pdd_sync(void* stream);

/* Corner turn [nspec][nchan] (in_dtype) -> [nchan][nspec] (out_dtype: PDD_F32,
 * or the input dtype for a raw byte transpose).
 * Replaces filterbank.get_spectra's reshape + `.T` + Spectra.__init__'s
 * astype('float') (formats/filterbank.py:153-157, formats/spectra.py:34) and
 * mockspecfil2subbands' per-block transpose (bin/mockspecfil2subbands.py:155-175). */
int pdd_corner_turn(const void* in, int in_dtype, int64_t nspec, int64_t nchan, int64_t ld_in,
                    void* out, int out_dtype, int64_t ld_out, void* stream);

/* Elementwise dtype conversion of a [rows][cols] array to float32
 * (Spectra.__init__ data.astype, formats/spectra.py:34, for C-ordered input). */
int pdd_convert_f32(const void* in, int in_dtype, int64_t rows, int64_t cols, int64_t ld_in,
                    float* out, int64_t ld_out, void* stream);

/* Per-channel statistic of x[C][N] -> out[C] (float32): mean / median (pad
 * values of Spectra.shift_channels 'mean'/'median', formats/spectra.py:83-86;
 * Spectra.masked maskvals, spectra.py:216-222), std / min / max
 * (Spectra.scaled / scaled2 per-channel terms, spectra.py:157-187). */
int pdd_channel_stats(const float* x, int64_t C, int64_t N, int64_t ld, int stat,
                      float* out, void* stream);

/* out[c][t] = X(c, t + bins[c]) for t < n_out, X = x inside [0,N), padvals[c]
 * (PDD_PAD_VALUE) or wrap (PDD_PAD_ROTATE) outside.
 * Replaces Spectra.shift_channels (formats/spectra.py:54-94) incl.
 * psr_utils.rotate (spectra.py:80). `out` must not alias `x`. */
int pdd_shift_pad(const float* x, int64_t C, int64_t N, int64_t ld, const int32_t* bins,
                  int pad_mode, const float* padvals, float* out, int64_t ld_out,
                  int64_t n_out, void* stream);

/* Fused shift + group sum: out[k][t] = sum_{c in group k} X(c, t + bins[c]),
 * groups = nsub contiguous blocks of C/nsub channels, t < n_out.
 * nsub == nchan-groups: Spectra.subband (formats/spectra.py:96-138);
 * nsub == 1: Spectra.dedisperse + channel sum, the dedispersed series of
 * bin/waterfaller.py:140 (spectra.py:229-260).  bins may be NULL (no shift). */
int pdd_shift_group_sum(const float* x, int64_t C, int64_t N, int64_t ld, const int32_t* bins,
                        int pad_mode, const float* padvals, int64_t nsub, float* out,
                        int64_t ld_out, int64_t n_out, void* stream);

/* out[c][j] = sum_{k<factor} x[c][j*factor + k], j < N/factor.
 * Replaces Spectra.downsample (formats/spectra.py:329-351). */
int pdd_downsample(const float* x, int64_t C, int64_t N, int64_t ld, int64_t factor,
                   float* out, int64_t ld_out, void* stream);
/* The same on 8-bit channel rows (a Spectra's unmodified raw bytes): exact
 * integer sums, written as float32; reads a quarter of the float32 image's
 * bytes.  Used by the DDplan executor (spectra.py:329-351 per DDstep). */
int pdd_downsample_u8(const uint8_t* x, int64_t C, int64_t N, int64_t ld, int64_t factor,
                      float* out, int64_t ld_out, void* stream);
/* The same co-add kept as uint16 (factor 1..4: sums <= 1020), the input of
 * the exact 16-bit sweep (PDD_U16) -- the DDplan executor's downsampled
 * 8-bit steps (formats/spectra.py:329-351 on raw 8-bit rows). */
int pdd_downsample_u8_u16(const uint8_t* x, int64_t C, int64_t N, int64_t ld, int64_t factor,
                          uint16_t* out, int64_t ld_out, void* stream);

/* Zero-DM filter: every spectrum minus its channel mean; integer data use
 * round-half-even of the float64 mean and wrap modulo 2^nbits, float32 data
 * stay float32.  Replaces bin/zero_dm_filter.py:30-50 (filter + write loop).
 * `out` may alias `in`. */
int pdd_zero_dm(const void* in, int dtype, int64_t nspec, int64_t nchan, int64_t ld,
                int layout, void* out, int64_t ld_out, void* stream);

/* Streaming prologue, one HBM pass over a time-major block [nspec][nchan]
 * (filterbank order, u8/u16/f32): corner turn + zero-DM in float mode
 * (zero_dm != 0: every spectrum minus its float64 channel mean, the
 * subtraction of bin/zero_dm_filter.py:30-39 without the integer cast) +
 * Spectra.downsample(factor) (formats/spectra.py:329-351; factor divides 64):
 *   out[c][j] = sum_{k<factor} (x[j*factor+k][c] - mean[j*factor+k]),
 * j < nspec / factor, out channel-major float32. */
int pdd_zdm_downsample(const void* in, int dtype, int64_t nspec, int64_t nchan, int64_t ld,
                       int64_t factor, int zero_dm, float* out, int64_t ld_out, void* stream);

/* The 8-bit prologue of the exact 16-bit sweep (streaming configs[4]): the
 * same zero-DM + downsample + corner turn in integer arithmetic,
 *   out[c][j] = offset + sum_{k<factor} z(x[j*factor+k][c]),  uint16, channel-major,
 * with m = the spectrum's channel mean rounded half-to-even (np.round, as
 * bin/zero_dm_filter.py:30-39) and z by mode:
 *   PDD_ZDM_NONE  z = x                  (no filter; plain downsample)
 *   PDD_ZDM_INT   z = x - m, signed      (integer zero-DM without the uint8 wrap)
 *   PDD_ZDM_WRAP  z = (x - m) mod 256    (the reference's uint8 result exactly)
 * 8-bit input with 16-byte-aligned rows (nchan % 16 == 0); offset must keep
 * every value in [0, 65535] (PDD_ZDM_INT: offset >= 255 factor).  For the
 * 16-bit sweep (values <= 1023): factor <= 2 for PDD_ZDM_INT (offset 255
 * factor), <= 4 otherwise (offset 0). */
enum { PDD_ZDM_NONE = 0, PDD_ZDM_INT = 1, PDD_ZDM_WRAP = 2 };
int pdd_zdm_int_downsample(const void* in, int dtype, int64_t nspec, int64_t nchan, int64_t ld,
                           int64_t factor, int mode, int offset, uint16_t* out, int64_t ld_out,
                           void* stream);

/* ---- SIGPROC filterbanks packed below a byte (nbits 1, 2 or 4) ----
 * Order within a byte is SIGPROC's: the first channel sits in the least
 * significant bits (4 bits: low nibble first, as formats/psrfits.py
 * unpack_4bit; 2 bits: fields at shifts 0, 2, 4, 6; 1 bit: bit 0 first).
 * Parity of the 1- and 2-bit orders with a reference reader is unpinned
 * (the reference reads neither). */
/* The general path: time-major packed rows in[nspec] of nchan nbits / 8 bytes,
 * ld_in_bytes apart -> time-major uint8 out[nspec][nchan] (rows ld_out apart),
 * for every consumer of an 8-bit block.  Any nchan with nchan nbits % 8 == 0,
 * any strides, nspec >= 0.  16 channels per thread (one 2 nbits-byte load,
 * one 16-byte store) where nchan % 16 == 0 and both pointers and strides are
 * aligned to those widths; one packed byte per thread otherwise. */
int pdd_unpack_bits(const void* in, int nbits, int64_t nspec, int64_t nchan, int64_t ld_in_bytes,
                    uint8_t* out, int64_t ld_out, void* stream);
/* pdd_zdm_int_downsample reading packed rows (streaming configs[4] on 1-, 2-
 * and 4-bit files): unpack + zero-DM + co-add by factor + corner turn in one
 * pass, no 8-bit intermediate.  For every mode, factor and offset the output
 * is bit for bit pdd_zdm_int_downsample's on the unpacked bytes: m is the
 * spectrum's channel mean (double(sum) / double(nchan), the sum taken exactly
 * over the bit fields) rounded half-to-even, PDD_ZDM_WRAP is mod 256 (uint8
 * arithmetic on the unpacked array), the trailing partial group is dropped.
 * Packed rows must be 16-byte aligned (in, ld_in_bytes and nchan nbits / 8
 * multiples of 16); with vmax = 2^nbits - 1, offset + factor vmax (255 factor
 * for PDD_ZDM_WRAP) <= 65535, and offset >= factor vmax for PDD_ZDM_INT.  For
 * the 16-bit sweep (values <= 1023) 4-bit data allow factor <= 64 without a
 * filter and <= 32 with PDD_ZDM_INT (offset 15 factor). */
int pdd_zdm_packed_int_downsample(const void* in, int nbits, int64_t nspec, int64_t nchan,
                                  int64_t ld_in_bytes, int64_t factor, int mode, int offset,
                                  uint16_t* out, int64_t ld_out, void* stream);

/* ---- waterfaller post-chain (Spectra.scaled / scaled2 / masked / smooth) ---- */
/* Whole-array statistics of x[C][N] into out4 (device float[4]):
 * {mean, population std, min, max}, float64 accumulation.
 * Replaces other.data.std() / other.data.max() (formats/spectra.py:156, 181). */
int pdd_global_stats(const float* x, int64_t C, int64_t N, int64_t ld, float* out4, void* stream);
/* out[c][t] = (x[c][t] - sub[c*sub_inc]) / div[c*div_inc] (inc 0 = broadcast).
 * Replaces the per-channel loops of Spectra.scaled (formats/spectra.py:157-162)
 * and Spectra.scaled2 (spectra.py:182-187). */
int pdd_scale_rows(const float* x, int64_t C, int64_t N, int64_t ld, const float* sub,
                   int64_t sub_inc, const float* div, int64_t div_inc, float* out, int64_t ld_out,
                   void* stream);
/* out[c][t] = mask[c][t] ? vals[c] : x[c][t]  (mask: uint8 0/1).
 * Replaces np.where(mask, maskvals, data) of Spectra.masked (formats/spectra.py:225-226). */
int pdd_masked_fill(const float* x, int64_t C, int64_t N, int64_t ld, const uint8_t* mask,
                    int64_t ld_mask, const float* vals, float* out, int64_t ld_out, void* stream);
/* Boxcar of `width` samples and height 1/sqrt(width), 'same' centring, per
 * channel, padded with padvals[c] (PDD_PAD_VALUE: number / 'mean' / 'median')
 * or wrapped (PDD_PAD_ROTATE: 'wrap').  Replaces Spectra.smooth
 * (formats/spectra.py:262-303; scipy.signal.convolve). `out` must not alias x. */
int pdd_smooth(const float* x, int64_t C, int64_t N, int64_t ld, int64_t width, int pad_mode,
               const float* padvals, float* out, int64_t ld_out, void* stream);

/* ---- batched DM sweep (new executor over utils/DDplan2b.py grids) ----
 * plane[d][t] = sum_c X(c, t + table[d][c]), t < n_out (defaults of
 * Spectra.dedisperse(dm, padval, trim=True) + channel sum, per DM trial,
 * formats/spectra.py:229-260 + bin/waterfaller.py:140).
 * The plan holds the device copy of the delay table and its per-block
 * extents; it is built once per (grid, channel count, dtype). */
typedef struct pdd_sweep_plan pdd_sweep_plan;

/* host_table: [D][C] int32, row d = the bins Spectra.dedisperse(dms[d])
 * would pass to shift_channels.  dtype: PDD_F32, PDD_U8 or PDD_U16 (samples
 * <= 1023) input. */
int pdd_sweep_plan_create(const int32_t* host_table, int64_t D, int64_t C, int dtype,
                          pdd_sweep_plan** plan);
/* The same with plan flags (pdd_sweep_plan_create = PDD_SWEEP_FACTOR):
 * PDD_SWEEP_FACTOR lets a single-group plan sweep factorised over groups of
 * 4 (or 2) adjacent channels when the plan's cost model says it pays: each
 * group's distinct relative-shift patterns are summed once (stage 1), and
 * every trial adds its pattern series at the group's base shift (stage 2).
 * Integer plans (PDD_U8 / PDD_U16, also through pdd_sweep_execute_ds) sum
 * the same integer samples as the channel-by-channel kernel: the plane is
 * bit-identical.  PDD_F32 plans regroup the float32 channel sum (within the
 * float32 bar; exact for integer-valued data).  Flags 0 forces the
 * channel-by-channel kernel.  Factorised plans take the plain and the
 * pieces layouts and column offsets; they do not chain
 * (pdd_subband_chain). */
#define PDD_SWEEP_FACTOR 1
/* with PDD_SWEEP_FACTOR: factorise whenever the windows fit, paying or not
 * (tests of small grids) */
#define PDD_SWEEP_FACTOR_FORCE 2
/* with PDD_SWEEP_FACTOR: groups of 2 channels only (default: 4 or 2, the
 * cheaper by the plan's cost model; 2 where a 4-channel group's pattern
 * windows do not fit one LDS chunk buffer) */
#define PDD_SWEEP_FACTOR_G2 4
#define PDD_SWEEP_FACTOR_G4 8  /* groups of 4 channels only */
/* with PDD_SWEEP_FACTOR: plane-aligned factorised tiles (default: each trial's
 * time tile is skewed by its delay at a mid-band reference group, so a
 * tile's pattern windows span less drift; the plane is identical) */
#define PDD_SWEEP_NO_SKEW 16
int pdd_sweep_plan_create_ex(const int32_t* host_table, int64_t D, int64_t C, int dtype, int flags,
                             pdd_sweep_plan** plan);
/* Channels per factor group of the plan (4 or 2; 0 = channel by channel) and, if
 * n_patterns is non-null, its stage-1 pattern count. */
int pdd_sweep_plan_factor(const pdd_sweep_plan* plan, int64_t* n_patterns);
/* Largest per-trial time-tile skew of a factorised plan's delay-aligned tiles
 * (samples of an eighth / quarter; 0: plane-aligned tiles or a channel plan),
 * and, if extra_tiles is non-null, the time tiles each segment adds for it. */
int pdd_sweep_plan_skew(const pdd_sweep_plan* plan, int64_t* extra_tiles);
/* x: [C][N] (ld) of the plan's dtype; out: [D][ld_out] float32.
 * For PDD_U8 with PDD_PAD_VALUE every padvals[c] must be an integer in
 * [0, 255] (checked on the host side by the caller).  PDD_U16 input: unsigned
 * 16-bit samples <= 1023 (e.g. the offset output of pdd_zdm_int_downsample),
 * swept exactly with the packed-u16 kernels. */
int pdd_sweep_execute(const pdd_sweep_plan* plan, const void* x, int64_t N, int64_t ld,
                      int pad_mode, const float* padvals, float* out, int64_t ld_out,
                      int64_t n_out, void* stream);
/* The same with two more input layouts/offsets (DM-sharded sweeps):
 *   piece == 0: x is channel-major [C][ld];
 *   piece == P > 0 (a power of two): x is [ceil(N/P)][C][P] -- the block an
 *     all-gather of per-rank channel-major time slices of P samples produces
 *     (sample s of channel c at x[(s/P)*C*P + c*P + s%P]);
 *   x_off: plane column t sums input samples t + x_off + table[d][c] (a column
 *     range [x_off, x_off + n_out) of the full sweep); pads apply outside
 *     [0, N) of x;
 *   out_bias: added to every plane value (e.g. -offset * C for offset input). 
 * Offsets and pieces need the interleaved tilings (every grid whose shift
 * span per trial block fits the LDS); sparser grids return an error. */
int pdd_sweep_execute_ex(const pdd_sweep_plan* plan, const void* x, int64_t N, int64_t ld,
                         int64_t piece, int64_t x_off, int pad_mode, const float* padvals,
                         float* out, int64_t ld_out, int64_t n_out, float out_bias,
                         void* stream);
/* The same over TIME-MAJOR input (file order): x is [N][ld_t] spectra, sample
 * s of channel c at x[s*ld_t + c], ld_t >= the plan's channels; x_off, pads
 * and out_bias as above.  A factorised plan's stage 1 reads the spectra
 * directly (8-bit input with x and ld_t multiples of the group size: the
 * group's channels as one 4- or 2-byte word per spectrum), so a caller that
 * holds the block in file order needs no pdd_corner_turn before the sweep.
 * Interleaved tilings only, as for pieces. */
int pdd_sweep_execute_tm(const pdd_sweep_plan* plan, const void* x, int64_t N, int64_t ld_t,
                         int64_t x_off, int pad_mode, const float* padvals, float* out,
                         int64_t ld_out, int64_t n_out, float out_bias, void* stream);
/* Staged execution of a factorised plan (pdd_sweep_plan_factor > 0, raw-rate
 * input) for pipelining: stage 1 (1: the pattern image, written into
 * `patterns`), stage 2 (2: the sweep, reading the pattern image stage 1 of the
 * same x / x_off / n_out wrote into `patterns`) or both (3), one segment (the
 * whole column range) per call, arguments as pdd_sweep_execute_ex.  Two
 * pattern buffers let stage 1 of the next block run on one stream while
 * stage 2 of this block runs on another (DMShardedSweep: CU-partitioned
 * streams, pdd_stream_create_cu_mask).  `pattern_bytes` must be >=
 * pdd_sweep_pattern_bytes(plan, n_out). */
int64_t pdd_sweep_pattern_bytes(const pdd_sweep_plan* plan, int64_t n_out);
int pdd_sweep_execute_stage(const pdd_sweep_plan* plan, const void* x, int64_t N, int64_t ld,
                            int64_t piece, int64_t x_off, int pad_mode, const float* padvals,
                            float* out, int64_t ld_out, int64_t n_out, float out_bias,
                            void* patterns, int64_t pattern_bytes, int stage, void* stream);
/* A stream whose kernels run only on the CUs set in `mask` (n_words 32-bit
 * words, bit i = CU i; hipExtStreamCreateWithCUMask) / its release. */
int pdd_stream_create_cu_mask(const uint32_t* mask, int n_words, void** stream);
int pdd_stream_destroy(void* stream);
/* Grouped sweep: n_grp independent channel groups of C channels each
 * (channels g*C .. g*C+C-1 of the input), every group with its own [D][C]
 * table: host_table is [n_grp][D][C].  One launch replaces n_grp sweeps --
 * the stage-1 subband passes of a DDplan step (Spectra.subband at each subDM,
 * formats/spectra.py:96-138, one group per subband) or the stage-2 sweeps of
 * its passes (one group per pass).  Trial d of group g is written to plane
 * row g*row_g + d*row_d. */
int pdd_sweep_plan_create_grouped(const int32_t* host_table, int64_t n_grp, int64_t D, int64_t C,
                                  int dtype, pdd_sweep_plan** plan);
int pdd_sweep_execute_grouped(const pdd_sweep_plan* plan, const void* x, int64_t N, int64_t ld,
                              int pad_mode, const float* padvals, float* out, int64_t ld_out,
                              int64_t n_out, int64_t row_g, int64_t row_d, void* stream);
/* Sweep of an 8-bit block downsampled by ds (2..4) on the fly: x8 is
 * channel-major [C_all][ld] uint8 at the raw rate (n_raw samples); the swept
 * series is Spectra.downsample(ds) of it (formats/spectra.py:329-351: N =
 * n_raw / ds co-adds, exact integers <= 1020), so the plan must be PDD_U16.
 * Grouped and ungrouped plans (ungrouped: row_g 0, row_d 1); pads act on the
 * downsampled series (integers <= 1023 or PDD_PAD_ROTATE).  Replaces
 * pdd_downsample_u8_u16 + pdd_sweep_execute(_grouped) of a DDplan step
 * (utils/DDplan2b.py:102-199 downsamp) without the downsampled copy. */
int pdd_sweep_execute_ds(const pdd_sweep_plan* plan, const uint8_t* x8, int64_t n_raw, int64_t ld,
                         int64_t ds, int pad_mode, const float* padvals, float* out,
                         int64_t ld_out, int64_t n_out, int64_t row_g, int64_t row_d,
                         void* stream);
/* Both stages of a subbanded DDplan step in two launches and no subband
 * plane: stage 1 (plan1: grouped, one group per subband, trials = the passes'
 * subDMs; PDD_U8 rows at ds 1 or PDD_U16 with x = 8-bit rows co-added by
 * ds 2..4 on the fly, as pdd_sweep_execute_ds) writes its rows -- trial d of
 * group g = stage-2 channel d * n_grp1 + g, i.e. the subbands of pass d --
 * directly as stage 2's float32 quarters image; stage 2 (plan2: PDD_F32,
 * grouped, one group per pass, delays >= 0) sweeps that image into out (trial
 * d of group g at row g*row_g + d*row_d, n_out columns).  pad2vals[c]: the
 * value pad of stage-2 channel c (Spectra.dedisperse padval on the subbanded
 * data).  Equals pdd_sweep_execute(_grouped/_ds) of stage 1 into a
 * [n_grp2*C2][N1] subband plane followed by pdd_sweep_execute_grouped of
 * stage 2 over it (formats/spectra.py:96-138 then :229-260 per pass).
 * Returns PDD_ENOCHAIN (-5), with nothing launched, for a block/grid it
 * cannot chain (a stage that needs more than one segment, or a stage-2 delay
 * span wider than an eighth of the block): run the two stages apart then.
 * Any other negative status (e.g. -2: scratch allocation failed) is an
 * error of this call. */
#define PDD_ENOCHAIN (-5)
int pdd_subband_chain(const pdd_sweep_plan* plan1, const void* x, int64_t n_raw, int64_t ld,
                      int64_t ds, int pad1_mode, const float* pad1vals,
                      const pdd_sweep_plan* plan2, const float* pad2vals, float* out,
                      int64_t ld_out, int64_t n_out, int64_t row_g, int64_t row_d, void* stream);
/* Extents used by the plan (for DESIGN/bench reporting): DM trials, channels,
 * DMs per block, time samples per block, LDS bytes per workgroup. */
int pdd_sweep_plan_info(const pdd_sweep_plan* plan, int64_t* info /*[8]*/);
/* Integer-input plans (PDD_U8, PDD_U16): the largest sample value the
 * caller's input (and integer pads) can hold, default 255 / 1023.  The
 * sweep adds two samples per 32-bit lane pair and converts every
 * floor(65535 / max_value) channels (at most 256), so a tighter bound means
 * fewer conversions; a sample above it gives wrong sums.  E.g. the
 * zero_dm_filter.py:30-39 uint8-wrap image co-added by 2 is <= 510. */
int pdd_sweep_plan_set_input_max(pdd_sweep_plan* plan, int max_value);
/* Test switches of a plan (parity tests and the C-ABI driver; both default
 * off).  poison: factorised plans fill their pattern image with 0xFF bytes
 * before stage 1 of every segment, so a stage-2 read of an element stage 1
 * did not write shows as a NaN / overflowed lane.  segment_bytes > 0: the
 * scratch budget of one time segment (default: 16 GiB, 80 GiB for factorised
 * plans, capped by free device memory), to run the multi-segment path on
 * small blocks. */
int pdd_sweep_plan_set_poison(pdd_sweep_plan* plan, int on);
int pdd_sweep_plan_set_segment_bytes(pdd_sweep_plan* plan, int64_t bytes);
int pdd_sweep_plan_destroy(pdd_sweep_plan* plan);
/* Measurement hooks (bench.py): with timing on, every sweep-kernel launch
 * of pdd_sweep_execute(_grouped) -- not the interleave pre-pass -- is
 * bracketed by its own pair of HIP events on the execute stream (no host
 * synchronisation; up to 1024 launches between reads).
 * pdd_sweep_timing_read waits for the last one and returns the SUM of the
 * bracketed durations and the number of launches since the previous read;
 * pdd_sweep_kernel_ms is the same sum alone. */
int pdd_sweep_set_timing(pdd_sweep_plan* plan, int on);
int pdd_sweep_timing_read(pdd_sweep_plan* plan, float* total_ms, int64_t* launches);
int pdd_sweep_kernel_ms(pdd_sweep_plan* plan, float* ms);

/* ---- single-pulse boxcar search over a DM-time plane (SURVEY.md §8(f)
 * rank 4; no reference search -- the boxcar is Pulse.smooth,
 * formats/pulse.py:217-241; definition in pypulsar_amd/search.py).
 * x: [D][n] float32 plane, row stride ld.  L: detrend chunk length. */
/* Per row and chunk of L samples (last may be short): mean and 1/std
 * (0 where std == 0), written to [D][ceil(n/L)] arrays. */
int pdd_sp_chunk_stats(const float* x, int64_t D, int64_t n, int64_t ld, int64_t L, float* mean,
                       float* istd, void* stream);
/* Boxcar S/N of every start and width (widths: HOST array, ascending,
 * 1..1025, at most 32) on the chunk-normalised rows; one candidate per
 * (row, window of 1024 starts) with S/N >= threshold, appended to cands as
 * int32 records {row, start, width, float-bits snr} through the device
 * counter *count (incremented for every candidate, stored while
 * < max_cands: the caller checks for overflow).  Record order is not
 * deterministic; the set is.
 * Streams: a row may continue into a second plane -- row d is
 * x[d][0:n] followed by x_next[d][0:n_next] (n % L == 0; its chunks use
 * mean_next/istd_next, [D][ceil(n_next/L)]) -- and only starts < n_starts
 * are searched, so block i of a stream is searched with the first columns
 * of block i+1 exactly as the one-shot plane would be.  n_next = 0 (and
 * null next pointers): a single plane. */
int pdd_sp_search(const float* x, int64_t D, int64_t n, int64_t ld, int64_t L, const float* mean,
                  const float* istd, const float* x_next, int64_t n_next, int64_t ld_next,
                  const float* mean_next, const float* istd_next, int64_t n_starts,
                  const int32_t* widths, int n_widths, float threshold, int32_t* cands,
                  int64_t max_cands, unsigned long long* count, void* stream);

/* ---- grouping of single-pulse candidates across DM row, time and width
 * (pypulsar_amd/spgroup.py; restated by brute force in
 * tests/spgroup_oracle.py).  A candidate is the record {row, start, width,
 * float-bits snr} of pdd_sp_search; its extent is [start, start + width).
 * Candidates a, b are linked when |row_a - row_b| <= row_tol and
 * max(start_a, start_b) - min(end_a, end_b) <= time_tol (negative: the
 * extents overlap); a group is a connected component of the links.
 * 0 <= row_tol <= 16, 0 <= time_tol <= 1023, 1 <= width <= 1025, start >= 0,
 * start + width + time_tol < 2^31, k < 2^31.  Canonical order: ascending by
 * (start / 1024, row, start, width, snr bits as int32). */
/* cands: DEVICE int32 [k][4], 16-byte aligned, in canonical order (the
 * kernels need the order of the cell key (start / 1024) * nrows + row only);
 * nrows > every row.  label[i] = the index of the first member of i's
 * group: the same for any scheduling.  Memory: the k labels, nothing
 * proportional to the plane.  k == 0: nothing is launched. */
int pdd_spg_label(const int32_t* cands, int64_t k, int64_t nrows, int row_tol, int time_tol,
                  int32_t* label, void* stream);
/* groups: DEVICE int32 [k][8], 16-byte aligned, written whole by the call:
 * at index g == label[g]: {members, best, row_lo, row_hi, start_lo, end_hi,
 * snr bits of best, 0} -- best: the index of the member of the highest S/N
 * compared as floats, the smallest index on a tie (a NaN is outside the
 * contract); start_lo = min start, end_hi = max (start + width); at every
 * other index: zeros.  Integer atomics only: the same bits for any
 * scheduling. */
int pdd_spg_summarise(const int32_t* cands, const int32_t* label, int64_t k, int32_t* groups,
                      void* stream);

/* ---- cut-outs of single-pulse candidates: the dedispersed frequency-time
 * image and the DM-time image of many candidates from one block of the file
 * (pypulsar_amd/cutout.py; restated by brute force in
 * tests/cutout_oracle.py).
 * x: DEVICE time-major block [n][C], row stride ld elements, PDD_U8 or
 * PDD_F32 (the file's order: no corner turn).  table: DEVICE int32
 * [rows][C] delay bins (delays.sweep_table).  padvals: DEVICE float32 [C],
 * or NULL for 0: what a sample outside rows 0..n-1 of the block contributes.
 * jobs: DEVICE int64 [J][5] = {t0, f, row0, bmin, bmax}: t0 the first raw
 * row of the image relative to the block's first row (negative allowed,
 * |t0| <= 2^40), f the samples summed per bin (1 <= f <= fmax), row0 the
 * job's first table row; bmin <= every entry of the job's ndm table rows
 * <= bmax (read by pdd_cutout_dmt only).
 * Limits: 1 <= nbin, ndm <= 1024, 1 <= fmax <= 1024, C fmax 255 < 2^31,
 * nsub divides C; anything else is refused (-1).  A job that breaks what is
 * stated about it (f, row0, bmin/bmax, span) touches no memory outside the
 * buffers: its image is NaN.
 * 8-bit input: float32(exact integer sum of the in-range samples) + the
 * float32 pad term; float32 input: float32 sums in a fixed order.  No
 * atomics: the same bits however the jobs are batched. */
/* out: DEVICE float32 [J][nsub][nbin],
 *   out[j][s][b] = sum_{c in subband s} sum_{k<f} X(c, t0 + b f + k + table[row0][c]),
 * subband s = channels s C/nsub .. (s+1) C/nsub - 1. */
int pdd_cutout_ft(const void* x, int dtype, int64_t n, int64_t C, int64_t ld, const int64_t* jobs,
                  int64_t J, const int32_t* table, int64_t rows, const float* padvals, int nbin,
                  int nsub, int fmax, float* out, void* stream);
/* out: DEVICE float32 [J][ndm][nbin],
 *   out[j][d][b] = sum_{all c} sum_{k<f} X(c, t0 + b f + k + table[row0 + d][c]).
 * span >= (nbin + ceil((bmax - bmin + 1) / f)) f of every job, <= 2^22: the
 * positions of a job's per-channel box sums.  work: DEVICE scratch of
 * work_bytes >= span C e bytes (e = 2 for PDD_U8 with fmax <= 257, else 4),
 * 4-byte aligned; as many jobs as fit it go through each pair of launches. */
int pdd_cutout_dmt(const void* x, int dtype, int64_t n, int64_t C, int64_t ld, const int64_t* jobs,
                   int64_t J, const int32_t* table, int64_t rows, const float* padvals, int nbin,
                   int ndm, int fmax, int64_t span, void* work, int64_t work_bytes, float* out,
                   void* stream);

/* ---- periodicity search of a DM-time plane (pypulsar_amd/periodicity.py;
 * the arithmetic of PrestoFFT.deredden, formats/prestofft.py:151-195, and
 * PrestoFFT.harmonic_sum, :98-113).  Spectra are interleaved (re, im)
 * float32 pairs with row stride ld in COMPLEX elements; nn = nfft / 2 bins of
 * a row are used (no Nyquist bin).  offs, lens: DEVICE int32 tables of the B
 * whitening blocks (periodicity.deredden_table; lens <= 256). */
/* out[d][t] = float32(double(x[d][t]) - mean_d) for t < n, 0 for
 * n <= t < nfft (out: [D][nfft], contiguous); mean_d accumulated in float64
 * in a fixed order (deterministic).  Zero padding after mean removal stands
 * in for PRESTO's pad-with-mean. */
int pdd_ps_prep(const float* x, int64_t D, int64_t n, int64_t ld, int64_t nfft, float* out,
                void* stream);
/* med[d][j] = median(P[offs[j] : offs[j] + lens[j]]) / ln 2, P = re*re + im*im
 * in float32; np.median's rule (even length: mean of the two middle values),
 * by exact selection.  med: [D][B]. */
int pdd_ps_block_medians(const float* spec, int64_t D, int64_t nn, int64_t ld, const int32_t* offs,
                         const int32_t* lens, int64_t B, float* med, void* stream);
/* The reference's whitening applied to powers: for block j < B - 1 and
 * offset i in it, lineval = med[j] + slope_j (0.5 (lens[j] + lens[j+1]) - i),
 * slope_j = (med[j+1] - med[j]) / (lens[j] + lens[j+1]); from offs[B-1] to nn
 * the last lineval of block B - 2.  powers_out[d][k] = P / lineval
 * ([D][nn], contiguous; bin 0 is 1); spec_out (may be null): the complex
 * spectrum times 1 / sqrt(lineval) ([D][nn] complex, contiguous; bin 0 is
 * 1 + 0j) -- the reference's return value.  Where lineval <= 0 or NaN (a
 * dead row) both are 0 (the reference gives inf / NaN).  B >= 2. */
int pdd_ps_normalise(const float* spec, int64_t D, int64_t nn, int64_t ld, const int32_t* offs,
                     const int32_t* lens, int64_t B, const float* med, float* powers_out,
                     float* spec_out, void* stream);
/* out[d][k] = sum_{h=1..nharm} powers[d][h k] for k < nn / nharm
 * (out: [D][nn / nharm], contiguous), float32, ascending h (numpy's += order:
 * bit-identical to the reference for equal input).  nharm 1..32. */
int pdd_ps_harmsum(const float* powers, int64_t D, int64_t nn, int64_t ld, int nharm, float* out,
                   void* stream);
/* All stages fused (harms: HOST array, ascending, 1..32, at most 8; thr: HOST
 * array, one float threshold per stage): the sums run cumulatively in
 * ascending h, so each stage's sum has the bits of pdd_ps_harmsum.  Bin k of
 * [rlo, nn / H) is a candidate of stage H when S_H[k] >= thr, S_H[k] >
 * S_H[k-1] and S_H[k] >= S_H[k+1] (neighbours outside the range: -inf).
 * Records int32 {row, k, H, float-bits S_H[k]} are appended through the
 * device counter *count exactly as by pdd_sp_search (always incremented,
 * stored while < max_cands: the caller checks for overflow). */
int pdd_ps_search(const float* powers, int64_t D, int64_t nn, int64_t ld, const int32_t* harms,
                  int n_harms, const float* thr, int64_t rlo, int32_t* cands, int64_t max_cands,
                  unsigned long long* count, void* stream);

/* ---- acceleration search in the Fourier domain (pypulsar_amd/accel.py;
 * PrestoFFT.interpolate, formats/prestofft.py:76-96, carried to drifting
 * signals).  spec: the whitened complex spectrum of pdd_ps_normalise,
 * interleaved (re, im) float32, row stride ld in COMPLEX elements, nn bins a
 * row; bins outside [0, nn) count as 0. */
/* powers[d][j][i] = |sum_{e=-hw[j]..hw[j]} F[d][k0 + e] t[j][phi][e]|^2 with
 * k0 = i >> 1, phi = i & 1, i < 2 nn (half-bin positions).  taps: DEVICE
 * float32 [nz][2][2 M + 1][2] = (re, im) of t[j][phi][e] at index M + e
 * (accel.template_bank); hw: HOST int32 [nz], 0 <= hw[j] <= M <= 512 (z values
 * are processed four at a time to the largest half-width of the four, so
 * taps beyond hw[j] must be 0); nz odd, <= 255.  powers: [D][nz][2 nn]
 * float32, contiguous.  float32 fused multiply-adds in a fixed order
 * (deterministic). */
int pdd_acc_correlate(const float* spec, int64_t D, int64_t nn, int64_t ld, const float* taps,
                      const int32_t* hw, int nz, int M, float* powers, void* stream);
/* Harmonic stages on the TOP harmonic's grid and the candidate search of
 * powers [D][nz][ni] (contiguous; J0 = (nz - 1) / 2, jc = j - J0).  harms:
 * HOST array, ascending, 1..16, at most 8; thr: HOST array, one float
 * threshold per stage.
 *   S_H[jc][i] = sum_{h=1..H} P[J0 + floor((jc h + H / 2) / H)][(i h + H / 2) / H]
 * (float32, ascending h from the h = 1 term; H / 2 an integer division).
 * Cell (j, i) with i >= 2 H rlo is a candidate of stage H when S >= thr, S >
 * its neighbours (j-1, i-1), (j-1, i), (j-1, i+1), (j, i-1) and S >= the
 * neighbours (j, i+1), (j+1, i-1), (j+1, i), (j+1, i+1); neighbours outside
 * [0, nz) x [2 H rlo, ni) count as -inf.  Records int32 {row, i, jc, H,
 * float-bits S, 0} are appended through the device counter *count exactly as
 * by pdd_ps_search (always incremented, stored while < max_cands: the caller
 * checks for overflow). */
int pdd_acc_search(const float* powers, int64_t D, int nz, int64_t ni, const int32_t* harms,
                   int n_harms, const float* thr, int64_t rlo, int32_t* cands, int64_t max_cands,
                   unsigned long long* count, void* stream);

/* ---- jerk search (pypulsar_amd/jerk.py; restated in tests/jerk_oracle.py).
 * vol: [nw][D][nz][ni] float32, contiguous: slab l = the powers
 * pdd_acc_correlate writes for all D rows with the taps of the jerk w_l = (l -
 * L0) dw (L0 = (nw - 1) / 2, lc = l - L0; J0, jc as above). */
/* Harmonic stages on the TOP harmonic's grid -- pdd_acc_search's rule in both
 * template axes -- and the candidate search of the volume.  harms, thr: HOST
 * arrays as for pdd_acc_search.
 *   S_H[lc][jc][i] = sum_{h=1..H} P[L0 + floor((lc h + H / 2) / H)][d]
 *                                  [J0 + floor((jc h + H / 2) / H)][(i h + H / 2) / H]
 * (float32, ascending h from the h = 1 term).  Cell (l, j, i) with i >= 2 H
 * rlo is a candidate of stage H when S >= thr, S > each of the 13 of its 26
 * neighbours that precede it in (l, j, i) order and S >= each of the 13 that
 * follow; neighbours outside [0, nw) x [0, nz) x [2 H rlo, ni) count as -inf
 * (nw = 1: pdd_acc_search's rule).  scratch: DEVICE, scratch_floats >= 3 D nz
 * ni floats (a ring of three S_H slabs; contents undefined afterwards).  nw
 * odd, <= 63; nz odd, <= 255.  Records int32[8] {row, i, jc, lc, H, float-bits
 * S, 0, 0} are appended through the device counter *count exactly as by
 * pdd_acc_search (always incremented, stored while < max_cands: the caller
 * checks for overflow). */
int pdd_jerk_search(const float* vol, int64_t D, int nw, int nz, int64_t ni, const int32_t* harms,
                    int n_harms, const float* thr, int64_t rlo, float* scratch,
                    int64_t scratch_floats, int32_t* cands, int64_t max_cands,
                    unsigned long long* count, void* stream);

/* ---- Fourier-domain interference zapping (pypulsar_amd/zap.py; restated in
 * tests/zap_oracle.py).  powers: whitened powers of pdd_ps_normalise, one
 * spectrum a row. */
/* out[k] = the rank-th smallest (1-based, 1 <= rank <= R) of powers[r ld + k],
 * r < R, for every k < nn: exact selection, the value returned is one of the
 * column's, whatever the ties (-0 counts as below +0).  1 <= R <= 64.  The
 * inputs are finite by construction (pdd_ps_normalise writes 0 for a dead
 * row): a NaN is outside the contract (the result of such a column is
 * unspecified, nothing else is affected). */
int pdd_zap_percentile(const float* powers, int64_t R, int64_t nn, int64_t ld, int rank,
                       float* out, void* stream);
/* bins: DEVICE int32 [nz][2], inclusive bin intervals [lo, hi], sorted,
 * disjoint, 1 <= lo <= hi < nn.  In each of the D rows powers[d ldp + k] = 1
 * for lo <= k <= hi -- the whitened mean level -- and, where spec is not
 * null (interleaved (re, im) float32, row stride lds in COMPLEX elements),
 * spec[d lds + k] = (0.70710677, 0.70710677), of unit power.  Nothing else is
 * written.  nz == 0 or D == 0: nothing is launched. */
int pdd_zap_apply(float* powers, int64_t ldp, float* spec, int64_t lds, int64_t D, int64_t nn,
                  const int32_t* bins, int64_t nz, void* stream);

/* ---- folding of plane rows at candidate periods and the search of the folds
 * over period / period-derivative offsets (pypulsar_amd/fold.py; restated in
 * tests/fold_oracle.py).  Phase is a 64-bit unsigned fraction of a turn with
 * wrap-around arithmetic.  A job is 4 int64 {row, P0, step, accel} (the last
 * three the bit patterns of unsigned values, fold.phase_steps):
 *   step  = round(f dt 2^64) mod 2^64,  accel = round(fd dt dt 2^64) mod 2^64,
 *   P0    = round(phi0 2^64) + step / 2 (the centre of sample 0).
 * Sample i of the row has P_i = P0 + i step + (i (i - 1) / 2) accel (mod
 * 2^64) and falls into bin ((P_i >> 32) * nbins) >> 32. */
/* The row is cut into npart parts of L = n / npart samples (the last
 * n - npart L samples are not folded).  Per job: prof[J][npart][nbins]
 * float64 sums of the samples per bin, cnt[J][npart][nbins] int32 sample
 * counts, sumsq[J][npart] float64 sums of squares.  Accumulation is float64
 * in no fixed order: exact (bit-identical to any order) on integer-valued
 * rows.  jobs: HOST copy, jobs_dev: the same J x 4 int64 on the device; a
 * row outside [0, D) is refused before anything is launched.  2 <= nbins <=
 * 256, 1 <= npart <= 128, npart nbins <= 8192, n < 2^31; J == 0: no-op. */
int pdd_fold_rows(const float* plane, int64_t D, int64_t n, int64_t ld, const int64_t* jobs,
                  const int64_t* jobs_dev, int64_t J, int npart, int nbins, double* prof,
                  int32_t* cnt, double* sumsq, void* stream);
/* For each job and every trial (ia, ib) of [-A, A] x [-B, B]: with N = npart
 * and m = 2 p + 1 - N, part p is shifted by
 *   s_p = floor((ia m N + 2 ib m m + N N) / (2 N N))      (floor division)
 * bins, the nearest bin to ia u + 4 ib u u, u = m / (2 N):
 *   S[b] = sum_p prof[p][(b + s_p) mod nbins] (ascending p), C[b] from cnt,
 *   chi2[ia][ib] = (sum over b ascending, C[b] > 0, of
 *                   (S[b] - C[b] mu)^2 / (C[b] var)) / (nbins - 1),
 * all float64 without contraction.  mu = tot / Ntot and var = q / Ntot - mu mu
 * with tot the sum over ascending p of (the sum over ascending b of
 * prof[p][b]), q the sum of sumsq over ascending p, Ntot the sample count;
 * var <= 0 gives chi2 = 0.  chi2: [J][2A+1][2B+1].  best[J][2] = (ia, ib) of
 * the first trial in the order (chi2 descending, |ib|, |ia|, ib, ia
 * ascending), best_chi2[J] its chi2, best_prof[J][nbins] / best_cnt[J][nbins]
 * its S and C.  A, B <= 256. */
int pdd_fold_search(const double* prof, const int32_t* cnt, const double* sumsq, int64_t J,
                    int npart, int nbins, int A, int B, double* chi2, int32_t* best,
                    double* best_chi2, double* best_prof, int32_t* best_cnt, void* stream);

/* ---- folding of periodicity candidates from the raw block into (sub-
 * integration, subband, phase) cubes and the DM refinement on such a cube
 * (pypulsar_amd/subfold.py; restated by brute force in
 * tests/subfold_oracle.py).
 * x: DEVICE time-major block [n][C], row stride ld elements, PDD_U8 or
 * PDD_F32 (the layout of pdd_cutout_*), whose first row is raw sample
 * t_first of a file of N samples.  table: DEVICE int32 [rows][C] delay bins
 * (delays.sweep_table at the raw dt, reference = the highest channel: every
 * entry >= 0).  A job is 8 int64 {P0, step, accel, L, i0, i1, row, bmax}:
 * the phase model of pdd_fold_rows (fold.phase_steps; f at raw sample 0),
 * b[c] = table[row][c], bmax = max_c b[c], n_out = N - bmax the trimmed
 * length of a single-DM sweep, L = n_out / npart.  Dedispersed sample
 * i < npart L has P_i = P0 + i step + (i (i - 1) / 2) accel (mod 2^64) and
 * bin(i) = ((P_i >> 32) * nbins) >> 32, shared by every channel; the rest is
 * dropped as in pdd_fold_rows.  Subband s = channels s C/nsub ..
 * (s+1) C/nsub - 1 in file order.  With p = i / L:
 *   cube[j][p][s][bin(i)] += sum_{c in s} x[i + b[c]][c]        float64
 *   cnt[j][p][bin(i)]     += 1   (per sample, not per channel)  int32
 *   chansum[j][c] += x[i + b[c]][c],  chansq[j][c] += x^2       float64
 * A call folds the samples i0 <= i < i1 of each job from the block it is
 * given and ADDS to the outputs, which pdd_subfold_zero (or the caller)
 * cleared: a file is folded block by block, consecutive blocks overlapping
 * by bmax rows.  Promised per job, checked on the HOST copy before anything
 * is launched: L >= 1, 0 <= i0 <= i1 <= npart L, 0 <= row < rows, and, where
 * i0 < i1, t_first <= i0 and i1 - 1 + bmax < t_first + n.  The kernel guards
 * every load: a job whose device table breaks bmax reads nothing outside the
 * block (such samples count as 0; the result is unspecified).
 * 8-bit input: integers on chip, then float64 adds of integers below 2^53:
 * every output is the exact integer, bit-identical for any scheduling and
 * any split into blocks.  float32 input: float64 sums in no fixed order.
 * Limits (refused, -1): 2 <= nbins <= 256, 1 <= npart <= 128, npart nbins <=
 * 8192, nsub nbins <= 8192, nsub divides C, n < 2^31, npart L < 2^31.  jobs:
 * HOST copy, jobs_dev: the same J x 8 int64 on the device.  J == 0: no-op.
 * tile_span: the largest (max - min) delay within any aligned group of 64
 * consecutive channels of any job's table row, or -1 where unknown (bmax is
 * taken): it only sizes the LDS in which 8-bit rows are staged; the kernel
 * checks every tile's own span and reads per lane where it does not fit, so
 * a wrong value costs time, never a result. */
int pdd_subfold_zero(double* cube, int32_t* cnt, double* chansum, double* chansq, int64_t J,
                     int64_t C, int npart, int nsub, int nbins, void* stream);
int pdd_subfold(const void* x, int dtype, int64_t n, int64_t C, int64_t ld, int64_t t_first,
                const int64_t* jobs, const int64_t* jobs_dev, int64_t J, const int32_t* table,
                int64_t rows, int npart, int nsub, int nbins, double* cube, int32_t* cnt,
                double* chansum, double* chansq, int64_t tile_span, void* stream);
/* DM refinement of J cubes.  trials: DEVICE int32 [J][2] = (ia, ib); rtab:
 * DEVICE int32 [J][ndm][nsub]; ntot: DEVICE int64 [J] = npart L.  Per job,
 * with s_p = the shift of part p of pdd_fold_search's formula (fold.trial_shift):
 *   sub[s][b] = sum_p cube[p][s][(b + s_p) mod nbins]   (ascending p),
 *   Cb[b]     = the same sum over cnt,
 *   subints[p][b] = sum_s cube[p][s][b]                 (ascending s, no shift),
 *   mu_c = chansum[c] / Ntot, var_c = chansq[c] / Ntot - mu_c mu_c,
 *   mu_s = sum_{c in s} mu_c, var_s = sum_{c in s} var_c (ascending c; 0 where Ntot = 0).
 * Ladder entry k reads subband s r = rtab[k][s] mod nbins bins further on;
 * with idx = (b + r) mod nbins and sums over ascending s:
 *   S_k[b] = sum_s sub[s][idx], E_k[b] = sum_s mu_s Cb[idx], V_k[b] = sum_s var_s Cb[idx],
 *   chi2[k] = (sum over b ascending, V_k[b] > 0, of (S_k[b] - E_k[b])^2 / V_k[b]) / (nbins - 1),
 * all float64 without contraction.  (The host makes rtab[k][s] =
 * floor((dms[k] - DM) u_s f nbins + 0.5) mod nbins, u_s the delay per unit DM
 * of the subband's centre relative to the highest channel: subfold.ladder_shifts.)
 * best[J]: the first k in the order (chi2 descending, |k - ndm / 2|
 * ascending, k ascending); best_chi2[J]; best_prof[J][nbins] = S_best;
 * best_cnt[J][nbins] int64 = sum_s Cb[idx] of the best entry (the (sample,
 * subband) pairs behind S_best[b]).  chi2: [J][ndm], sub: [J][nsub][nbins],
 * subints: [J][npart][nbins].  1 <= ndm <= 1024 and the limits of pdd_subfold. */
int pdd_subfold_dm(const double* cube, const int32_t* cnt, const double* chansum,
                   const double* chansq, const int64_t* ntot, const int32_t* trials,
                   const int32_t* rtab, int64_t J, int64_t C, int npart, int nsub, int nbins,
                   int ndm, double* chi2, int32_t* best, double* best_chi2, double* best_prof,
                   int64_t* best_cnt, double* sub, double* subints, void* stream);

/* ---- fast-folding (FFA) search of a DM-time plane for long periods
 * (pypulsar_amd/ffa.py; restated in tests/ffa_oracle.py).  A step of the plan
 * searches base periods p0 = b_lo .. b_hi - 1 bins on the series downsampled
 * by f.
 *
 * Prepare: y[i] = x[f i] + x[f i + 1] + .. + x[f i + f - 1], float32, ascending
 * (a sum: integer rows stay integer), i < n_ds = n / f.  The series is cut
 * into nchunk = max(1, n_ds / L) chunks of L samples, the last one running to
 * the end; mean_c is the float64 mean of chunk c and ctr_c the mean index of
 * its samples.  base(i) = mean_c + (mean_{c+1} - mean_c) (i - ctr_c) / (ctr_{c+1}
 * - ctr_c) for ctr_c <= i < ctr_{c+1}, mean_0 before ctr_0 and mean_{nchunk-1}
 * from ctr_{nchunk-1} on; y'[i] = float32(double(y[i]) - base(i)) and
 * sigma^2 = sum(y'^2) / n_ds - (sum(y') / n_ds)^2 in float64 (sigma = 0 where
 * that is not positive).  Sums of float64 run in a fixed order (deterministic).
 *
 * Transform of base period p0: M = n_ds / p0 rows y'[r p0 .. r p0 + p0) and
 * zero rows up to Mp = 2^K = max(2, next power of two >= M).  The transform
 * of one row is the row; two transformed half blocks head, tail of m / 2 rows
 * merge into m rows
 *   out[s][b] = head[s >> 1][b] + tail[s >> 1][(b + ((s + 1) >> 1)) mod p0],
 * one float32 add per element and stage: bit-identical to the NumPy
 * restatement for any input.  Trial s < Mp - 1 of the full transform is the
 * fold at period (p0 + s / (Mp - 1)) bins.
 *
 * Score of a profile x of b = p0 bins: P[i] = x[0] + .. + x[i] and T = P[b - 1]
 * in float32 (any association: exact for integer-valued profiles below 2^24),
 * c(0) = 0, c(i) = P[i - 1].  For each width w of `widths` (ascending) with
 * w <= max(1, floor(ducy_max b)) and w < b:
 *   S_w = max over b0 < b of  c(b0 + w) - c(b0)                 (b0 + w <= b)
 *                             (T - c(b0)) + c(b0 + w - b)        (otherwise),
 *   snr_w = (S_w - w T / b) / (sigma sqrt(M w (1 - w / b)))       (float64; the
 *           device multiplies by the reciprocals of b and of the denominator);
 * the entry is float32 of the largest snr_w and the index of its width (the
 * narrower on ties); 0 and index 0 where sigma == 0 or no width is admitted. */
/* Host only (no GPU): info[4] = {M, K, kpass, npass} of base period p0 on a
 * series of n_ds samples -- the K stages run as npass launches of
 * pdd_ffa_pass, kpass stages each (the last one the rest), sized so that two
 * buffers of 2^kpass rows of p0 floats fit the 160 KiB of LDS.  2 <= p0 <=
 * 1024, 2 p0 <= n_ds < 2^31. */
int pdd_ffa_plan_info(int64_t n_ds, int p0, int64_t* info);
/* y[d][i] (i < n / f, contiguous rows) and mean[d][c] of the chunks of L
 * downsampled samples, from rows x[d] of stride ld.  D < 65536. */
int pdd_ffa_downsample(const float* x, int64_t D, int64_t n, int64_t ld, int64_t f, int64_t L,
                       float* y, double* mean, void* stream);
/* In place y -> y' with the means of pdd_ffa_downsample; part: [D][nchunk][2]
 * float64 work area (the chunks' sums of y' and y'^2); sigma[d]. */
int pdd_ffa_detrend(float* y, int64_t D, int64_t n_ds, int64_t L, const double* mean, double* part,
                    double* sigma, void* stream);
/* Pass `pass` (0 .. npass - 1) of the transforms of the D np problems (row d,
 * base period p_lo + i), problem q = d np + i; base periods whose transform
 * has fewer passes are skipped.  Pass 0 reads the rows of y ([D][n_ds], row stride ld); a
 * later pass reads ws_in and a pass before the last writes ws_out, both
 * [D np][slot] float32 with slot >= Mp p0 for every base period that uses
 * them (two buffers alternate where npass > 2).  The last pass of a base
 * period scores its profiles: snr / widx [D][ntrial] at trial toff[i] + s (toff:
 * DEVICE int64 [np]; entries outside [0, ntrial) are not written); snr and
 * widx null: no score.  prof (test hook, np == 1, may be null): the finished
 * [D][Mp][p0] profiles.  widths: HOST int32 array, ascending, at most 16.
 * D np < 65536. */
int pdd_ffa_pass(const float* y, int64_t D, int64_t n_ds, int64_t ld, int p_lo, int np, int pass,
                 const float* ws_in, float* ws_out, int64_t slot, const double* sigma,
                 const int64_t* toff, const int32_t* widths, int n_widths, double ducy_max,
                 float* snr, uint8_t* widx, int64_t ntrial, float* prof, void* stream);
/* Trial k of snr [D][ntrial] (row stride ld) is a candidate when snr[k] >=
 * threshold, snr[k] > snr[k-1] and snr[k] >= snr[k+1] (neighbours outside the
 * row: -inf).  Records int32 {row, k, width index, float-bits snr} are
 * appended through the device counter *count exactly as by pdd_ps_search
 * (always incremented, stored while < max_cands: the caller checks for
 * overflow). */
int pdd_ffa_search(const float* snr, const uint8_t* widx, int64_t D, int64_t ntrial, int64_t ld,
                   float threshold, int32_t* cands, int64_t max_cands, unsigned long long* count,
                   void* stream);

/* ---- RFI excision on the raw time-major block (pypulsar_amd/rfi.py; restated
 * in tests/rfi_oracle.py).  raw: [nint ptsperint][C] 8-bit or float32 (dtype
 * PDD_U8 / PDD_F32), row stride ld elements, cut into nint intervals of
 * P = ptsperint samples (16 <= P <= 2^23). */
/* Pass (a) over channels c0 .. c0 + nc - 1: avg[i][c] and std[i][c] (float64,
 * [nint][C], only those columns written) of every (interval, channel) --
 * 8 bits: from the exact integer sums S1 = sum x, S2 = sum x^2 as
 * double(S1) / double(P) and sqrt(double(P S2 - S1 S1) / double(P P)); float32:
 * from float64 sums -- and rows[(c - c0) nint + i][P] (float32, contiguous):
 * the samples of the cell minus a constant near their mean (the mean of the
 * first <= 64, rounded to an integer for 8 bits; bins k >= 1 of a transform
 * of the row do not depend on it).  nvar[(c - c0) nint + i] = P var (float64). */
int pdd_rfi_stats_prep(const void* raw, int dtype, int64_t nint, int64_t C, int64_t ld,
                       int64_t ptsperint, int64_t c0, int64_t nc, float* rows, double* avg,
                       double* std, double* nvar, void* stream);
/* Pass (b): spec = the real-to-complex transform of `rows`, [nrows][P / 2 + 1]
 * interleaved (re, im) float32, contiguous, 16-byte aligned; nrows = nc nint.
 * pow[i][c0 + row / nint] (float64, [nint][C]) = max_{k=1..P/2} |spec[row][k]|^2
 * / nvar[row], 0 where nvar[row] == 0; i = row % nint. */
int pdd_rfi_stats_power(const float* spec, int64_t nrows, int64_t ptsperint, const double* nvar,
                        int64_t nint, int64_t C, int64_t c0, double* pow, void* stream);
/* In place on data [n][C] (row stride ld): sample (t, c) becomes fill[c] when
 * bit c % 32 of bitmap[(t0 + t) / ptsperint][c / 32] is set (bitmap: uint32
 * [nint][ceil(C / 32)], bits of channels >= C clear; fill: [C] of the data's
 * type).  Rows of intervals >= nint are left alone. */
int pdd_rfi_apply(void* data, int dtype, int64_t n, int64_t C, int64_t ld, int64_t t0,
                  int64_t ptsperint, const uint32_t* bitmap, int64_t nint, const void* fill,
                  void* stream);

/* ---- PSRFITS search-mode subints -> [nchan][N] float32 (SURVEY.md §8(f)
 * rank 3).  Replaces psrfits.unpack_4bit (formats/psrfits.py:37-50),
 * PsrfitsFile.read_subint (:67-107: ((data*scales)+offsets)*weights in
 * float32) and get_spectra (:140-183: concatenation, transpose, skip/trunc,
 * band flip).  raw: nsub consecutive SUBINT table rows as stored (row_bytes
 * each, big-endian; DATA at byte data_off of a row); nbits 4/8/16/32;
 * wso: [nsub][3][nchan] float32 scales, offsets, weights; output row
 * c' = flip ? nchan-1-c : c holds samples s0 .. s0+N-1 of the concatenated
 * subints. */
int pdd_psrfits_subints(const uint8_t* raw, int64_t nsub, int64_t row_bytes, int64_t data_off,
                        int nbits, int64_t nsblk, int64_t nchan, const float* wso, int64_t s0,
                        int64_t N, int flip, float* out, int64_t ld_out, void* stream);

/* ---- PSRFITS search-mode subints -> the stream's time-major raw block
 * out[n][nchan] (rows ld_out elements apart), channels in file order, no band
 * flip.  rows: nsub consecutive SUBINT table rows as stored (row_bytes each,
 * big-endian); DATA, [nsblk][npol][nchan] samples of nbits 4 (low nibble
 * first) / 8 (uint8) / 16 (int16) / 32 (float32), starts data_off bytes into
 * a row; scl_off, offs_off, wts_off are the byte offsets of DAT_SCL and
 * DAT_OFFS ([npol][nchan] float32) and DAT_WTS ([nchan] float32) in a row,
 * read from the rows themselves, or -1: not applied (1, 0, 1).  Output row
 * j < n is sample g = s0 + j of the concatenated subints (subint g / nsblk,
 * spectrum g % nsblk).
 *   PDD_F32: ((v scl[c]) + offs[c]) wts[c] in float32, in that order, of
 *     polarisation pol0 (bit for bit pdd_psrfits_subints' values); npol_sum
 *     == 2: (((v0 scl0[c]) + offs0[c]) + ((v1 scl1[c]) + offs1[c])) wts[c]
 *     of polarisations pol0 and pol0 + 1.
 *   PDD_U8: v where wts[c] != 0 (or weights are not applied), else 0; only
 *     with nbits <= 8, npol_sum == 1 and scl_off == offs_off == -1.
 * Refused (non-zero, nothing written): null pointers, another nbits, 4-bit
 * with odd npol nchan, s0 + n > nsub nsblk, a column running past row_bytes,
 * pol0 + npol_sum > npol, ld_out < nchan, PDD_U8 outside its conditions.
 * n == 0 returns 0 and writes nothing. */
int pdd_psrfits_block(const uint8_t* rows, int64_t nsub, int64_t row_bytes, int64_t data_off,
                      int64_t scl_off, int64_t offs_off, int64_t wts_off, int nbits, int64_t nsblk,
                      int64_t nchan, int npol, int pol0, int npol_sum, int64_t s0, int64_t n,
                      int out_code, void* out, int64_t ld_out, void* stream);

/* ---- Injection of synthetic pulsars and bursts into a raw time-major block
 * (pypulsar_amd/inject.py builds the job tables; restated in
 * tests/inject_oracle.py).  In place on data [n][C] (rows ld
 * elements apart, PDD_U8 or PDD_F32) whose row 0 is absolute sample t0.  With
 * G = ceil(C / PDD_INJECT_GROUP), job j < J and channel c < C:
 *   phase  uint64  [J][C][2]      P0, step: the phase at sample 0 and per
 *                                 sample, in units of 2^-64 turns
 *   drift  float64 [J][C][2]      k2 (per channel), k3 (the job's, repeated)
 *   range  int64   [J][C + G][2]  lo, hi: the job touches samples lo <= i < hi
 *                                 of channel c; entry C + g: an interval that
 *                                 holds those of channels 256 g .. 256 g + 255
 *                                 (tiles it misses are skipped)
 *   tables float32 [J][C][B + 1]  the profile at phases b / B; entry B is the
 *                                 one read beyond the last (entry 0 again for
 *                                 a periodic job, 0 for a burst)
 * The cell of absolute sample i = t0 + row and channel c gets, from every job
 * with lo <= i < hi, in job order,
 *   p   = P0 + i step (wrapping) + U(x x (k2 + x k3)),  x = (double) i,
 *         U(d) = (uint64)((d - floor(d)) 2^64), a difference of 1.0 counting
 *         as 0; every operation one IEEE operation in this order
 *   b   = p >> (64 - log2 B),  w = float((p >> (40 - log2 B)) & 0xffffff) 2^-24
 *   acc = acc + (T[b] + (T[b + 1] - T[b]) w)            (float32, from 0)
 * and becomes x + acc (PDD_F32) or min(vmax, max(0, floor((float(x) + acc) +
 * u))) (PDD_U8), u = float(h >> 8) 2^-24, h = fmix(fmix(fmix(lo32(i) ^ seed) ^
 * hi32(i) ^ 0x9e3779b9) ^ (c 0x27d4eb2f)) in 32-bit arithmetic, fmix being
 * MurmurHash3's finaliser.  A cell no job covers keeps its value: it is
 * not accessed, except that where four adjacent channels of a row go as one
 * dword or 16-byte access an uncovered cell beside a covered one is read and
 * written back unchanged (so no other writer may own it during the call).
 * Refused with -1, nothing touched: a null pointer (job tables: only when J >
 * 0), another dtype, n < 0, C < 1, ld < C, t0 < 0, t0 + n > 2^52, J outside
 * 0..PDD_INJECT_MAX_JOBS, B no power of two in 64..4096, seed outside
 * 0..2^32 - 1, vmax outside 1..255.  n == 0 or J == 0: returns 0. */
#define PDD_INJECT_GROUP 256
#define PDD_INJECT_MAX_JOBS 64
int pdd_inject(void* data, int dtype, int64_t n, int64_t C, int64_t ld, int64_t t0,
               const uint64_t* phase, const double* drift, const int64_t* range,
               const float* tables, int J, int B, int64_t seed, int vmax, void* stream);

/* pdd_inject with pulsars in Keplerian orbits (pypulsar_amd/inject.py builds
 * the tables; restated in tests/inject_orbit_oracle.py).  The
 * first fifteen arguments, the cell rule and the refusals are pdd_inject's.
 * A job j with an orbit (pb, x, e, omega, t0; the elements and the Roemer
 * delay D(t) of pdd_orbit_resample below) has the phase
 *   Phi(t) = phi0 + f t + fd t^2 / 2 + fdd t^3 / 6 - f (D(t) - D(0)),
 * whose last term Q = f (D - D(0)), in turns, is periodic in the orbital phase
 * psi = (t - t0) / pb and comes from a table of one orbit:
 *   ophase uint64  [J][C]   O0: psi of sample 0 in channel c, in units of
 *                           2^-64 orbits (read only for jobs with an orbit)
 *   ometa  int64   [J][3]   HOST array: m (-1: the job has no orbit and
 *                           follows pdd_inject's rule bit for bit; else 6..22:
 *                           its table has M + 1 = 2^m + 1 knots), ostep (psi
 *                           per sample, in 2^-64 orbits, the uint64's bits)
 *                           and the byte offset of the job's table in qtab
 *   qtab   float64 [qlen]   DEVICE, 8-byte aligned: per such job M + 1 knots
 *                           Q(k / M), k = 0..M, knot M repeating knot 0
 * For a job with an orbit the phase of a cell is, every operation one IEEE
 * operation in this order,
 *   psi = O0 + i ostep                                      (wrapping uint64)
 *   k   = psi >> (64 - m)
 *   w   = (double)((psi >> (32 - m)) & 0xffffffff) 2^-32    (exact)
 *   q   = qtab[k] + (qtab[k + 1] - qtab[k]) w               (float64)
 *   p   = P0 + i step + U(x x (k2 + x k3)) - U(q)           (wrapping)
 * and everything after p is pdd_inject's.  k is the top m bits of psi, so k +
 * 1 <= M whatever ophase holds, and a table must lie inside [0, qlen): no
 * element outside qtab[0..qlen) is read.  The orbit's values (ophase, qtab)
 * are device data and are NOT otherwise checked (pypulsar_amd.inject validates
 * the orbit, beta <= 0.1).  A launch in which some job has an orbit takes
 * tiles of 32 rows (pdd_inject: 64); the bits do not depend on the tiling.
 * With every m == -1 the call is pdd_inject's, launch included.  Refused with
 * -1, nothing touched, before any device call: what pdd_inject refuses; a null
 * ometa (J > 0); an m outside 6..22 and not -1; with some m >= 0: a null
 * ophase or qtab, a qtab that is not 8-byte aligned, a table offset that is
 * negative or no multiple of 8, a table that runs past qlen. */
#define PDD_INJECT_ORBIT_MIN_M 6
#define PDD_INJECT_ORBIT_MAX_M 22
int pdd_inject_orbit(void* data, int dtype, int64_t n, int64_t C, int64_t ld, int64_t t0,
                     const uint64_t* phase, const double* drift, const int64_t* range,
                     const float* tables, int J, int B, int64_t seed, int vmax,
                     const uint64_t* ophase, const int64_t* ometa, const double* qtab,
                     int64_t qlen, void* stream);

/* ---- sideband search for binaries shorter than the observation
 * (pypulsar_amd/sideband.py; Ransom, Cordes & Eikenberry 2003; restated in
 * tests/sideband_oracle.py).  powers: whitened powers of pdd_ps_normalise,
 * [D][nn] float32 with row stride ld; rlo as for pdd_ps_search. */
/* One mini-FFT length L = 2^log2L (5..14) a call.  stride = L >> shift (shift
 * 0..3); where nn - rlo >= L a row has nseg = (nn - rlo - L) / stride + 1
 * segments, segment j starting at lo = rlo + j stride (the fewer than stride
 * bins left below nn are not searched), otherwise none.  Of every segment,
 * with x_i = min(P[lo + i], clip) (clip > 0; clip == 0: x_i = P[lo + i]) and
 * A_k = sum_i x_i exp(-2 pi i i k / L), k = 0..L/2, in float32:
 *   M[2k]     = L |A_k|^2 / A_0^2
 *   M[2k + 1] = (pi^2 / 16) L |A_k - A_{k+1}|^2 / A_0^2
 * for k < L/2 (the half-bin grid q = 0..L-1; a segment with A_0 <= 0, a dead
 * row, has M = 0), and for the stages harms (HOST array, ascending, 1..8, at
 * most 4; thr: HOST array, one float threshold per stage)
 *   S_H[q] = sum_{h=1..H} M[h q],  q < L / H   (float32, ascending h).
 * q of [qlo, L / H) is a candidate of stage H when S_H[q] >= thr, S_H[q] >
 * S_H[q-1] and S_H[q] >= S_H[q+1] (neighbours outside the range: -inf); 1 <=
 * qlo <= L / 8.  twiddle: DEVICE float32 [L/2][2] = (cos, sin)(2 pi j / L),
 * 8-byte aligned (sideband.twiddle_table: float64, rounded once).  mini: null,
 * or DEVICE [D][nseg][L] float32 that receives M (the same bits on every
 * launch).  Records int32[6] {row, log2L, lo, q, H, float-bits S_H[q]} are
 * appended, in no particular order, through the device counter *count exactly
 * as by pdd_ps_search (always incremented, stored while < max_cands: the
 * caller checks for overflow).  No column >= nn of a row is read.  Refused
 * with -1, nothing launched: a null pointer, ld < nn, rlo < 1, log2L, shift,
 * nharm, harms or qlo outside their ranges, clip < 0.  D == 0 or nseg == 0:
 * returns 0. */
int pdd_sb_search(const float* powers, int64_t D, int64_t nn, int64_t ld, int64_t rlo, int log2L,
                  int shift, float clip, const int32_t* harms, int nharm, const float* thr,
                  int qlo, const float* twiddle, float* mini, int32_t* cands, int64_t max_cands,
                  int64_t* count, void* stream);

/* ---- coherent orbit demodulation (pypulsar_amd/orbit.py; the operation of the
 * reference's bin/demodulate.py for a bank of trial orbits; restated in
 * tests/orbit_oracle.py).  A time series row[0..n) of sampling time dt is
 * resampled into the pulsar's frame by T Keplerian templates at once; the
 * [T][n] result is searched and folded like a DM-time plane. */
/* orbits: DEVICE float64 [T][5] = pb (s), x (projected semi-major axis, light
 * seconds), e (in [0, 1)), omega (rad), t0 (time of periastron in s after
 * sample 0; for e = 0 the ascending node).  The Roemer delay is
 *   D(t) = x [(cos E - e) sin omega + sin E sqrt(1 - e^2) cos omega],
 *   E - e sin E = 2 pi (t - t0) / pb
 * (for e = omega = 0: x sin(2 pi (t - t0) / pb)), and output sample j (pulsar
 * time j dt) is taken at the input position p_j = t_j / dt with
 *   t_j - (D(t_j) - D(0)) = j dt,     so p_0 = 0.
 * Templates are meant to have beta = x (2 pi / pb) / (1 - e) <= 0.1, a bound
 * on |dD/dt| below which p is strictly increasing; orbit values are device
 * data and are NOT checked here (pypulsar_amd.orbit validates them).  p is
 * evaluated in float64 (Newton on Kepler's equation inside Newton on p, to
 * well below 1e-9 samples) at the knots j = k K only, k = 0 .. nk - 1, nk = (n
 * - 1) / K + 2, K a power of two in 1..256; for j = k K + i, 0 <= i < K:
 *   w = (double) i / (double) K                       (exact)
 *   p = p_k + (p_{k+1} - p_k) w                       (one IEEE float64
 *                                                      operation each)
 * The caller picks K so that A K^2 / 8 stays within its error budget, A = x (2
 * pi / pb)^2 dt / ((1 - e)^3 (1 - beta)^3) bounding |d2p/dj2| (orbit.py:
 * knot_spacing, 1e-3 samples).  The sample at p:
 *   PDD_ORBIT_NEAREST  out = row[floor(p + 0.5)]      (the reference's
 *                                                      drop / duplicate)
 *   PDD_ORBIT_LINEAR   i0 = floor(p), f = (float)(p - (double) i0),
 *                      out = a + (b - a) f in float32, a = row[i0], b = row[i0
 *                      + 1]; where i0 == n - 1: out = row[n - 1]
 * and in either mode a position outside [0, n - 1] (or a NaN) gives `fill`:
 * no element outside [0, n) of the row is read.  out: DEVICE [T][n] float32,
 * rows ld_out elements apart (elements n.. of a row are not written).  knots:
 * null, or DEVICE float64 [T][nk] that receives the p_k; the bits of out and
 * knots are the same on every launch, with or without the dump, and for any
 * split of the templates over launches.  One launch serves all T templates, on
 * a grid of ceil(n / tile) T workgroups, tile = (min(2045, 16384 / K) - 1) K
 * output samples (at least 2044).  Refused with -1, nothing launched: a null
 * row, orbits or out, n < 2 or n >= 2^31, T < 0, ld_out < n, dt <= 0, K no
 * power of two in 1..256, another mode, ceil(n / tile) T >= 2^31 (the caller
 * splits T).  T == 0: returns 0. */
#define PDD_ORBIT_NEAREST 0
#define PDD_ORBIT_LINEAR 1
int pdd_orbit_resample(const float* row, int64_t n, double dt, const double* orbits, int64_t T,
                       int K, int mode, float fill, float* out, int64_t ld_out, double* knots,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDD_H */
