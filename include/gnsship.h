/*
 * gnsship.h — C ABI of the MI355X-native GNSS acquisition + tracking correlator engine.
 *
 * This is the drop-in boundary.  Everything behind it is HIP code for gfx950;
 * everything in front of it is plain C: opaque handles, plain pointers and sizes, int status
 * codes.  No exceptions, no exit(), no torch / STL types cross this boundary.
 *
 * What each group of entry points replaces in the reference (ShingoNishimoto/gnss_sim_receiver,
 * a GNSS-SDR v0.0.19 fork; paths relative to its root):
 *
 *  gnsship_corr_*       Cpu_Multicorrelator_Real_Codes
 *                         (src/algorithms/tracking/libs/cpu_multicorrelator_real_codes.h:37-61,
 *                          .cc:36-167), i.e. volk_gnsssdr_32f_xn_resampler_32f_xn +
 *                          volk_gnsssdr_32fc_32f_rotator_dot_prod_32fc_xn, as called from
 *                          dll_pll_veml_tracking::do_correlation_step (dll_pll_veml_tracking.cc:1037-1062).
 *  gnsship_batch_*      The same correlation for many (channel, epoch) jobs in one launch: what
 *                         GNU Radio's thread-per-channel scheduling does across all channels.
 *  gnsship_acq_*        pcps_acquisition::set_local_code (pcps_acquisition.cc:175-208),
 *                         update_grid_doppler_wipeoffs (:295-302), acquisition_core (:600-871),
 *                         max_to_input_power_statistic / first_vs_second_peak_statistic (:496-597).
 *  gnsship_trk_*        dll_pll_veml_tracking::{start_tracking, general_work} (dll_pll_veml_tracking.cc:
 *                         643-883, 1728-2094) for many channels, the loop on the device.
 *  gnsship_comm_*       The flowgraph's fan-out of one signal-conditioner output to every channel
 *                         (gnss_flowgraph.cc:1127-1136) across GPUs: one RCCL communicator over
 *                         xGMI, the IF block broadcast from the reading rank, per-PRN acquisition
 *                         results all-gathered.
 *
 * Threading: handles are not re-entrant; distinct handles may be used from distinct threads
 * (each context owns one HIP stream).  All *_run calls are synchronous unless named *_launch.
 */
#ifndef GNSSHIP_H
#define GNSSHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: gnsship_trk_conf gained `rotator` and `if_hz` (a caller built against version 1 passes a shorter
 * struct — bindings compare gnsship_abi_version() with the header they were built from at load time). */
#define GNSSHIP_ABI_VERSION 2

/* ---- status codes (reference: bool-always-true + LOG/throw; here explicit) ---- */
#define GNSSHIP_OK 0
#define GNSSHIP_E_INVAL (-1)   /* bad argument / shape */
#define GNSSHIP_E_NOMEM (-2)   /* device or host allocation failed */
#define GNSSHIP_E_DEVICE (-3)  /* HIP runtime error (message in gnsship_last_error) */
#define GNSSHIP_E_STATE (-4)   /* call order violated (e.g. run before set_local_code) */
#define GNSSHIP_E_RCCL (-5)    /* RCCL (collective) error (message in gnsship_last_error)   */

/* ---- IF sample formats (reference item types: gr_complex, cshort, ibyte/cbyte) ---- */
#define GNSSHIP_FMT_CF32 0 /* interleaved float32 I,Q  (gr_complex)            */
#define GNSSHIP_FMT_CI16 1 /* interleaved int16  I,Q  (lv_16sc_t / cshort)      */
#define GNSSHIP_FMT_CI8 2  /* interleaved int8   I,Q  (ibyte/cbyte), no scaling  */
/* Read by the signal conditioner only (gnsship_cond_run); every other entry point rejects them.
 * Real-sampled IF, one value per sample, imaginary part 0, no scaling: the Freq_Xlating_Fir_Filter
 * adapter's input_item_type float / short / byte (freq_xlating_fir_filter.cc:118-159). */
#define GNSSHIP_FMT_RF32 3 /* float32 */
#define GNSSHIP_FMT_RI16 4 /* int16   */
#define GNSSHIP_FMT_RI8 5  /* int8    */
/* Bit-packed items: a byte holds 8/bits fields, bits = 2 or 4.  Field j in stream order sits at bit
 * offset bits*j (LSB_FIRST) or 8 - bits*(j + 1) (MSB_FIRST) and is a two's-complement integer s; the
 * sample value is 2s + 1 (MAP_2S1) or s (MAP_S).  REAL: one field per sample; IQ: fields 2m, 2m + 1 are
 * re, im of sample m; QI: im, re. */
#define GNSSHIP_FMT_PACKED_REAL 0
#define GNSSHIP_FMT_PACKED_IQ 1
#define GNSSHIP_FMT_PACKED_QI 2
#define GNSSHIP_FMT_PACKED_LSB_FIRST 0
#define GNSSHIP_FMT_PACKED_MSB_FIRST 1
#define GNSSHIP_FMT_PACKED_MAP_2S1 0
#define GNSSHIP_FMT_PACKED_MAP_S 1
#define GNSSHIP_FMT_PACKED(bits, components, order, map) (0x100 | ((bits) << 4) | ((components) << 2) | ((order) << 1) | (map))
#define GNSSHIP_FMT_IS_PACKED(fmt) (((fmt) & ~0xff) == 0x100)
#define GNSSHIP_FMT_PACKED_BITS(fmt) (((fmt) >> 4) & 0xf)
#define GNSSHIP_FMT_PACKED_COMPONENTS(fmt) (((fmt) >> 2) & 0x3)
#define GNSSHIP_FMT_PACKED_ORDER(fmt) (((fmt) >> 1) & 0x1)
#define GNSSHIP_FMT_PACKED_MAP(fmt) ((fmt) & 0x1)
/* The reference's packed file sources (byte items, little-endian host):
 * Two_Bit_Packed_File_Signal_Source, sample_type real / iq / qi, big_endian_bytes false (LSB_FIRST) / true
 * (unpack_2bit_samples.cc:150-207); Nsr_File_Signal_Source (unpack_byte_2bit_samples.cc:50-65);
 * Two_Bit_Cpx_File_Signal_Source (unpack_byte_2bit_cpx_samples.cc:77-90, re = bits 7:6, im = 5:4, ...);
 * Four_Bit_Cpx_File_Signal_Source, sample_type iq / qi (unpack_byte_4bit_samples.cc:44-65). */
#define GNSSHIP_FMT_TWO_BIT_PACKED(components, order) GNSSHIP_FMT_PACKED(2, components, order, GNSSHIP_FMT_PACKED_MAP_2S1)
#define GNSSHIP_FMT_NSR GNSSHIP_FMT_PACKED(2, GNSSHIP_FMT_PACKED_REAL, GNSSHIP_FMT_PACKED_LSB_FIRST, GNSSHIP_FMT_PACKED_MAP_S)
#define GNSSHIP_FMT_TWO_BIT_CPX GNSSHIP_FMT_PACKED(2, GNSSHIP_FMT_PACKED_IQ, GNSSHIP_FMT_PACKED_MSB_FIRST, GNSSHIP_FMT_PACKED_MAP_2S1)
#define GNSSHIP_FMT_FOUR_BIT_CPX(components) GNSSHIP_FMT_PACKED(4, components, GNSSHIP_FMT_PACKED_LSB_FIRST, GNSSHIP_FMT_PACKED_MAP_2S1)

#define GNSSHIP_MAX_TAPS 8

/* ---- rotator dot-product variant (volk_gnsssdr_32fc_32f_rotator_dot_prod_32fc_xn) ----
 * The reference's correlations depend on which volk_gnsssdr variant its dispatcher picks
 * (volk_gnsssdr_rank_archs.c): the generic C kernel (:66-98; VOLK_GENERIC set, or no AVX) or the
 * u_avx/a_avx kernel (:155-316; any AVX host without a volk_gnsssdr_config override): 16 phasors
 * advanced by normalise(inc^16), renormalised every 64 iterations.  The two differ by up to 1e-2
 * relative at 50 Msps with a 7 MHz IF, so the engine reproduces either one, selected per job / per
 * tracking engine.  Generic: the phasor chain and the serial float sum per tap component are
 * replayed in the reference's order (bit-identical taps; GNSSHIP_JOB_ROTATOR_TREE selects the faster
 * anchored tree sums for batch jobs).  AVX: all 16 phasor lanes are replayed and continued with the
 * reference's float products, in u_avx's accumulation order in the tracking engines (bit-identical taps).
 * Default in every binding (Python TrkConf.defaults, the C++ mirror's Dll_Pll_Conf, tools/gnsship_rx):
 * GNSSHIP_ROTATOR_AUTO, i.e. what the reference itself would run on this host. */
#define GNSSHIP_ROTATOR_GENERIC 0
#define GNSSHIP_ROTATOR_AVX 1
#define GNSSHIP_ROTATOR_AUTO (-1) /* what volk_gnsssdr dispatches on this host (gnsship_rotator_dispatch) */
/* gnsship_corr_job::flags bits */
#define GNSSHIP_JOB_HIGH_DYN 1     /* high-dynamics resampler + rotator (set_high_dynamics_resampler) */
#define GNSSHIP_JOB_ROTATOR_AVX 2  /* the AVX rotator variant (ignored with GNSSHIP_JOB_HIGH_DYN) */
/* Generic rotator with the anchored parallel sums (the phasor bit-identical at every renormalisation
 * point, the taps summed as a tree: within 1e-5 of the exact sum of the reference's float products,
 * not in its serial order).  Without this flag (and without _AVX / _HIGH_DYN) a job runs the
 * generic rotator in the reference's own order — one phasor chain and one serial float sum per tap
 * component, bit-identical taps (one workgroup per job, latency ≈ the N-step chain). */
#define GNSSHIP_JOB_ROTATOR_TREE 4
/* The variant volk_gnsssdr's dispatcher would select for the rotator dot-product on this host:
 * VOLK_GENERIC set in the environment -> generic; an entry for the kernel in the volk_gnsssdr
 * preferences file ($VOLK_CONFIGPATH or $HOME/.volk_gnsssdr/volk_gnsssdr_config) -> that entry
 * (its aligned and unaligned names are taken as the same variant: a_avx / u_avx and generic are
 * reproduced; any other entry, e.g. generic_reload, returns GNSSHIP_E_INVAL naming it in
 * gnsship_rotator_dispatch_detail); otherwise the AVX variant when the CPU has AVX.
 * *variant = GNSSHIP_ROTATOR_GENERIC / _AVX. */
int gnsship_rotator_dispatch(int* variant);
/* What the last gnsship_rotator_dispatch call on this thread matched (the environment, the
 * preferences file and its entry, or the CPU), as text. */
int gnsship_rotator_dispatch_detail(char* buf, int cap);

typedef struct gnsship_ctx gnsship_ctx;
typedef struct gnsship_corr gnsship_corr;
typedef struct gnsship_batch gnsship_batch;
typedef struct gnsship_acq gnsship_acq;

/* ------------------------------------------------------------------------------------------ */
/* Context: one HIP device + one stream + a code bank.                                        */
/* ------------------------------------------------------------------------------------------ */
int gnsship_abi_version(void);
int gnsship_device_count(int* n_devices);
int gnsship_ctx_create(int device, gnsship_ctx** out);
int gnsship_ctx_destroy(gnsship_ctx* ctx);
const char* gnsship_last_error(const gnsship_ctx* ctx);
int gnsship_ctx_sync(gnsship_ctx* ctx);
/* hipStream_t of the context, as void*, so a caller can order its own work against ours. */
int gnsship_ctx_stream(gnsship_ctx* ctx, void** stream);
/* HIP events recorded on the context stream (slots 0..15), for in-stream kernel timing. */
int gnsship_ctx_event_record(gnsship_ctx* ctx, int slot);
int gnsship_ctx_event_elapsed_ms(gnsship_ctx* ctx, int slot_begin, int slot_end, float* ms);

/* Device buffers (HBM).  The IF sample stream lives in one of these. */
int gnsship_dev_alloc(gnsship_ctx* ctx, size_t bytes, void** dev_ptr);
int gnsship_dev_free(gnsship_ctx* ctx, void* dev_ptr);
int gnsship_dev_upload(gnsship_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);
int gnsship_dev_download(gnsship_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);

/* Code bank: local code replicas (float, one value per code sample, e.g. 1023 for GPS C/A,
 * 8184 for Galileo E1 sinBOC(1,1) at 2 samples/chip).  Jobs refer to a code by its id.
 * Replaces the borrowed pointer of set_local_code_and_taps (cpu_multicorrelator_real_codes.cc:53-63):
 * the code is COPIED to the device. */
int gnsship_code_set(gnsship_ctx* ctx, int code_id, const float* code, int code_length);
int gnsship_code_count(gnsship_ctx* ctx, int* n_codes);

/* Local code replica generators (product side; reference src/algorithms/libs/ *_signal_replica.cc). */
/* gps_l1_ca_code_gen_float (gps_sdr_signal_replica.cc:113): dest[1023] = ±1 */
int gnsship_gps_l1_ca_code_gen_float(float* dest, int32_t prn, uint32_t chip_shift);
/* gps_l1_ca_code_gen_complex_sampled (:145): dest = n complex (code in imag); returns n or <0 */
int gnsship_gps_l1_ca_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t sampling_freq, uint32_t chip_shift);
/* beidou_b1i_code_gen_float (beidou_b1i_signal_replica.cc:113): dest[2046] = ±1 */
int gnsship_beidou_b1i_code_gen_float(float* dest, int32_t prn, uint32_t chip_shift);
/* beidou_b1i_code_gen_complex_sampled (:142): dest = n complex (code in real); returns n or <0 */
int gnsship_beidou_b1i_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t sampling_freq, uint32_t chip_shift);
/* gps_l5i_code_gen_float / gps_l5q_code_gen_float (gps_l5_signal_replica.cc:175, :244): dest[10230] = ±1,
 * PRN 1..32 (GNSSHIP_E_INVAL otherwise) */
int gnsship_gps_l5i_code_gen_float(float* dest, int32_t prn);
int gnsship_gps_l5q_code_gen_float(float* dest, int32_t prn);
/* gps_l5i_code_gen_complex_sampled (:193, code in real) / gps_l5q_code_gen_complex_sampled (:262, code in
 * imag): dest = n complex, chip index ceil(ts·(i+1)/tc) − 1 in float; returns n or <0 */
int gnsship_gps_l5i_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t sampling_freq);
int gnsship_gps_l5q_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t sampling_freq);
/* beidou_b3i_code_gen_float (beidou_b3i_signal_replica.cc:168): dest[10230] = ±1, PRN 1..63 (GNSSHIP_E_INVAL otherwise) */
int gnsship_beidou_b3i_code_gen_float(float* dest, int32_t prn, uint32_t chip_shift);
/* beidou_b3i_code_gen_complex_sampled (:196): dest = n complex (code in real), the B1I sampling rule; returns n or <0 */
int gnsship_beidou_b3i_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t sampling_freq, uint32_t chip_shift);
/* gps_l2c_m_code_gen_float (gps_l2c_signal_replica.cc:57): the L2 CM code, dest[10230] = ±1 (1 − 2·bit), PRN 1..50;
 * GNSSHIP_E_INVAL otherwise (the reference writes all +1 there) */
int gnsship_gps_l2c_m_code_gen_float(float* dest, int32_t prn);
/* gps_l2c_m_code_gen_complex_sampled (:75): dest = n complex (code in imag), chip index ceil(ts·(i+1)/tc) − 1 in
 * float; returns n or <0 */
int gnsship_gps_l2c_m_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t sampling_freq);
/* galileo_e5_a_code_gen_complex_primary / galileo_e5_b_… (galileo_e5_signal_replica.cc:31-93, :125-187): dest =
 * 10230 complex, chips ±1.  signal_id "5I" / "5Q" ("7I" / "7Q"): that component in the real part, the imaginary part
 * zero; "5X" ("7X"): the I component in the real part and the Q component in the imaginary part.  PRN 1..50 and one of
 * those signal ids, GNSSHIP_E_INVAL otherwise (the reference leaves dest untouched there). */
int gnsship_galileo_e5_a_code_gen_complex_primary(float* dest, int32_t prn, const char* signal_id);
int gnsship_galileo_e5_b_code_gen_complex_primary(float* dest, int32_t prn, const char* signal_id);
/* galileo_e5_a_code_gen_complex_sampled / galileo_e5_b_… (:96-122, :190-216): dest = n complex.  The primary is
 * sampled by resampler() (gnss_signal_replica.cc:275-290): chip (int)((1/fs·(i + 1))·10.23e6 + 1) − 1 in float, the
 * last sample forced to the last chip, and not at all when sampling_freq == 10230000; then rotated by
 * ((10230 − chip_shift) % 10230)·n / 10230 samples.  Returns n or <0. */
int gnsship_galileo_e5_a_code_gen_complex_sampled(float* dest, uint32_t prn, const char* signal_id, int32_t sampling_freq, uint32_t chip_shift);
int gnsship_galileo_e5_b_code_gen_complex_sampled(float* dest, uint32_t prn, const char* signal_id, int32_t sampling_freq, uint32_t chip_shift);
/* The four primaries as the tracker's code-bank replicas: dest[10230] = ±1, PRN 1..50 */
int gnsship_galileo_e5a_i_code_gen_float(float* dest, int32_t prn);
int gnsship_galileo_e5a_q_code_gen_float(float* dest, int32_t prn);
int gnsship_galileo_e5b_i_code_gen_float(float* dest, int32_t prn);
int gnsship_galileo_e5b_q_code_gen_float(float* dest, int32_t prn);
/* Secondary codes as '0' / '1' strings with a terminating NUL.  I components (Galileo_E5a.h:3581, Galileo_E5b.h:53):
 * dest[21] / dest[5], one fixed code each.  Q (pilot) components: dest[101], one 100-chip code per PRN — E5b-Q for
 * PRN 1..50, E5a-Q for PRN 1..47 (GALILEO_E5A_Q_SECONDARY_CODE ends there; the reference has no pattern for PRN
 * 48..50, and neither has this library: GNSSHIP_E_INVAL). */
int gnsship_galileo_e5a_i_secondary_code(char* dest);
int gnsship_galileo_e5b_i_secondary_code(char* dest);
int gnsship_galileo_e5a_q_secondary_code(char* dest, int32_t prn);
int gnsship_galileo_e5b_q_secondary_code(char* dest, int32_t prn);
/* glonass_l1_ca_code_gen_complex (glonass_l1_signal_replica.cc:25-77): the one GLONASS C/A code, 511 chips ±1,
 * rotated left by chip_shift.  _float: dest[511]; _complex: dest = 511 complex, the code in the real part. */
int gnsship_glonass_l1_ca_code_gen_float(float* dest, uint32_t chip_shift);
int gnsship_glonass_l1_ca_code_gen_complex(float* dest, uint32_t chip_shift);
/* glonass_l1_ca_code_gen_complex_sampled (:83-123): dest = n = (int)(fs / 1000) complex (code in real), chip index
 * ceil(ts·(i+1)/tc) − 1 in float, the last sample forced to the last chip; returns n or <0 */
int gnsship_glonass_l1_ca_code_gen_complex_sampled(float* dest, int32_t sampling_freq, uint32_t chip_shift);
/* glonass_l2_signal_replica.cc: the same code under the L2 names */
int gnsship_glonass_l2_ca_code_gen_float(float* dest, uint32_t chip_shift);
int gnsship_glonass_l2_ca_code_gen_complex(float* dest, uint32_t chip_shift);
int gnsship_glonass_l2_ca_code_gen_complex_sampled(float* dest, int32_t sampling_freq, uint32_t chip_shift);
/* GLONASS_PRN (GLONASS_L1_L2_CA.h:134): *k = the FDMA frequency channel (−7…+6) of PRN (orbital slot) 1..24, and 8 for
 * the reference's test entry PRN 0; GNSSHIP_E_INVAL for any other PRN.  The carrier of channel k is
 * 1602 MHz + k·562.5 kHz on L1 and 1246 MHz + k·437.5 kHz on L2. */
int gnsship_glonass_freq_channel(int32_t prn, int32_t* k);
/* samples per code period: (int)(fs / (chip_rate / code_len)) as the generators compute it */
int gnsship_code_samples_per_code(int32_t chip_rate, int32_t code_len, int32_t fs);

/* ------------------------------------------------------------------------------------------ */
/* Per-channel correlator: mirror of Cpu_Multicorrelator_Real_Codes.                          */
/* ------------------------------------------------------------------------------------------ */
/* init(max_signal_length_samples, n_correlators)  (cpu_multicorrelator_real_codes.cc:36-50) */
int gnsship_corr_create(gnsship_ctx* ctx, int max_signal_length_samples, int n_correlators, gnsship_corr** out);
/* set_local_code_and_taps(code_length_chips, local_code_in, shifts_chips)  (:53-63) */
int gnsship_corr_set_local_code_and_taps(gnsship_corr* c, int code_length_chips, const float* local_code_in, const float* shifts_chips);
/* set_high_dynamics_resampler (:163-167).  Default false, as Dll_Pll_Conf::high_dyn (dll_pll_conf.h:80). */
int gnsship_corr_set_high_dynamics_resampler(gnsship_corr* c, int enable);
/* Which volk_gnsssdr rotator variant the volk_gnsssdr_32fc_32f_rotator_dot_prod_32fc_xn call inside
 * Carrier_wipeoff_multicorrelator_resampler (:123-124) runs as: GNSSHIP_ROTATOR_GENERIC (the handle's
 * default; serial order, bit-identical taps), _AVX (u_avx: 16 phasor lanes) or _AUTO (what the
 * dispatcher would pick on this host, gnsship_rotator_dispatch; E_INVAL if it names a variant the
 * engine does not reproduce).  The C++ / Python mirrors default to _AUTO. */
int gnsship_corr_set_rotator(gnsship_corr* c, int variant);
/* Carrier_wipeoff_multicorrelator_resampler(...)  (:103-126).  `sig` is `fmt` samples; if
 * sig_on_device != 0 it is a device pointer (e.g. into a gnsship_dev_alloc ring), else host.
 * corr_out receives n_correlators complex<float> (2 floats each).  Synchronous. */
int gnsship_corr_run(gnsship_corr* c, const void* sig, int fmt, int sig_on_device,
    float rem_carrier_phase_in_rad, float phase_step_rad, float phase_rate_step_rad,
    float rem_code_phase_chips, float code_phase_step_chips, float code_phase_rate_step_chips,
    int signal_length_samples, float* corr_out);
/* free()  (:147-160) */
int gnsship_corr_destroy(gnsship_corr* c);

/* ------------------------------------------------------------------------------------------ */
/* Batched correlation: many (channel, epoch) jobs per launch.                                */
/* ------------------------------------------------------------------------------------------ */
/* One job = one call of Carrier_wipeoff_multicorrelator_resampler for one channel-epoch.
 * NCO arguments carry the same meaning and float type as the reference call
 * (dll_pll_veml_tracking.cc:1041-1048): code phases are in code SAMPLES (chips × samples/chip). */
typedef struct gnsship_corr_job {
    int64_t sample_offset;   /* first IF sample of this epoch in the device sample buffer      */
    int32_t n_samples;       /* correlation length (vector_length)                            */
    int32_t code_id;         /* code bank id                                                   */
    int32_t n_taps;          /* 1..GNSSHIP_MAX_TAPS                                            */
    int32_t flags;           /* GNSSHIP_JOB_HIGH_DYN | GNSSHIP_JOB_ROTATOR_AVX | _TREE           */
    float rem_carrier_phase_rad;
    float phase_step_rad;
    float phase_rate_step_rad;
    float rem_code_phase_chips;
    float code_phase_step_chips;
    float code_phase_rate_step_chips;
    float shifts_chips[GNSSHIP_MAX_TAPS];
} gnsship_corr_job; /* 80 bytes */

int gnsship_batch_create(gnsship_ctx* ctx, int max_jobs, gnsship_batch** out);
/* Copy job descriptors host→device (validated on the host: shapes, code ids, bounds). */
int gnsship_batch_set_jobs(gnsship_batch* b, const gnsship_corr_job* jobs, int n_jobs, int64_t n_buffer_samples);
/* Enqueue the correlation of all jobs on the context stream; results stay on the device.
 * dev_samples: device IF buffer in `fmt`; n_buffer_samples bounds every job. Asynchronous. */
int gnsship_batch_launch(gnsship_batch* b, const void* dev_samples, int fmt);
/* Profiling split of gnsship_batch_launch: stages bit0 = rotator-anchor replay (NCO arguments
 * only), bit1 = correlation (+ chunk reduction).  3 == gnsship_batch_launch. */
#define GNSSHIP_STAGE_ANCHORS 1
#define GNSSHIP_STAGE_CORRELATE 2
int gnsship_batch_launch_stages(gnsship_batch* b, const void* dev_samples, int fmt, int stages);
/* Wait for the last launch and copy results: out[j*2*GNSSHIP_MAX_TAPS + 2*t + {0,1}] = tap t of job j. */
/* Correlate b and, inside the same launch, replay the rotator anchors of `next` (another batch of the
 * same context; NULL for none) — the double-buffered form of batch_launch for a pair of batches
 * alternated on the context stream, with no cross-stream event per launch.  b's own anchors come
 * from the previous launch that named it as `next` (or are computed first).  Do not mix with
 * gnsship_batch_launch_stages on the same batches. */
int gnsship_batch_launch_pipelined(gnsship_batch* b, const void* dev_samples, int fmt, gnsship_batch* next);
/* Three-batch ring form (A, B, C, A, ...): correlate b, finish the anchor replay of `next` and run
 * the first half of `next2`'s (each job's replay chain split at its middle renormalisation block),
 * so every launch carries half a replay chain per batch instead of a whole one.  next / next2 may
 * be NULL; next2 == NULL is gnsship_batch_launch_pipelined. */
int gnsship_batch_launch_pipelined2(gnsship_batch* b, const void* dev_samples, int fmt, gnsship_batch* next, gnsship_batch* next2);
int gnsship_batch_results(gnsship_batch* b, float* out);
/* Device pointer of the result array (n_jobs × GNSSHIP_MAX_TAPS complex<float>). */
int gnsship_batch_results_device(gnsship_batch* b, void** dev_out);
int gnsship_batch_destroy(gnsship_batch* b);

/* ------------------------------------------------------------------------------------------ */
/* PCPS acquisition.                                                                          */
/* ------------------------------------------------------------------------------------------ */
/* Mirror of the Acq_Conf fields the core reads (acq_conf.h:33-81). */
typedef struct gnsship_acq_conf {
    int64_t fs_in;              /* sampling rate [Sps] (resampled_fs when no resampler)    */
    int32_t fft_size;           /* d_fft_size = consumed samples (sampled_ms == ms_per_code) */
    int32_t doppler_max;        /* [Hz]                                                       */
    int32_t doppler_step;       /* [Hz]                                                       */
    int32_t doppler_center;     /* [Hz]                                                       */
    int32_t max_dwells;         /* non-coherent dwells accumulated into the grid              */
    int32_t use_cfar;           /* 1: max_to_input_power_statistic, 0: first_vs_second_peak   */
    int32_t samples_per_chip;   /* ceil(fs / chip_rate)                                       */
    float samples_per_code;     /* samples_per_ms * ms_per_code                               */
    int32_t max_prns;           /* number of local-code slots (PRNs searched per call)        */
    int32_t consumed_samples;   /* d_consumed_samples (:71): input samples per dwell, the rest of
                                   the fft_size buffer zero-padded (sampled_ms != ms_per_code:
                                   fft_size = 2 x consumed, :84-91); 0 = fft_size              */
    int32_t bit_transition_flag; /* code in the second half after N/2 zeros, grid rows = the
                                   second half of |IFFT|^2 (:187-192, :663-664)                 */
    float resampler_ratio;       /* acquisition resampler decimation (Acq_Conf::resampler_ratio,
                                   acq_conf.cc:91-107); 0 or 1 = no resampler. Acq_delay_samples
                                   is scaled by it and reduced by the latency (:686-687)        */
    uint32_t resampler_latency_samples; /* (taps - 1) / 2 of the resampler FIR (gnss_flowgraph.cc:1113) */
} gnsship_acq_conf;

/* What acquisition_core leaves in Gnss_Synchro + block members (pcps_acquisition.cc:683-696). */
typedef struct gnsship_acq_result {
    uint32_t doppler_index;      /* winning Doppler bin                                       */
    uint32_t code_index;         /* indext: winning FFT sample index                          */
    int32_t doppler_hz;          /* Acq_doppler_hz                                            */
    float peak;                  /* grid maximum (or first peak)                             */
    float input_power;           /* d_input_power (CFAR) / second peak (first_vs_second)     */
    float test_statistic;        /* d_test_statistics                                         */
    double acq_delay_samples;    /* fmod(indext, samples_per_code)·resampler_ratio − latency   */
} gnsship_acq_result;

int gnsship_acq_create(gnsship_ctx* ctx, const gnsship_acq_conf* conf, gnsship_acq** out);
/* Rebuild the Doppler wipeoff table (update_grid_doppler_wipeoffs): row i is exp(j*phi_n),
 * phi accumulated in float32 exactly as volk_gnsssdr_s32f_sincos_32fc_generic. */
int gnsship_acq_set_grid(gnsship_acq* a, int doppler_max, int doppler_step, int doppler_center);
/* set_local_code (:175-208): `code` is the sampled code, complex<float>: fft_size/2 values with
 * bit_transition_flag, else consumed_samples values (zero-padded in front to fft_size); FFT + conj on device. */
int gnsship_acq_set_local_code(gnsship_acq* a, int prn_slot, const float* code);
/* update_grid_doppler_wipeoffs_step2 (:305-312), make_2_steps: nb2 bins around the step-one Doppler.
 * Results then carry the step-two Doppler (:553-556); with CFAR the statistic divides by
 * step_one_input_power, as the reference leaves d_input_power at its step-one value (:516-525).
 * gnsship_acq_set_grid returns to step one. */
int gnsship_acq_set_grid_step2(gnsship_acq* a, float doppler_center_step_two, float doppler_step2, int num_doppler_bins_step2,
    float step_one_input_power);
/* acquisition_core over prn slots [0, n_prns): one dwell of fft_size samples, all bins.
 * results[n_prns]; grid (optional, host, n_prns*n_bins*fft_size floats) receives |IFFT|^2. */
int gnsship_acq_run(gnsship_acq* a, const void* sig, int fmt, int sig_on_device, int n_prns,
    gnsship_acq_result* results, float* grid);
int gnsship_acq_num_bins(gnsship_acq* a, int* n_bins);
/* The transform layout the handle chose at create for its fft_size N (read-only; for tests and tooling
 * that must know which kernels a size runs). */
typedef struct gnsship_acq_layout {
    int32_t kind;       /* 0: one-workgroup LDS transform, 1: four-step, 2: huge                */
    int32_t P;          /* register points per column, N = P x row_len (0 for kind 0)           */
    int32_t row_len;    /* M, the LDS row transform's length (N for kind 0)                     */
    int32_t n_passes;   /* Stockham passes of the row plan                                      */
    int32_t radix[16];  /* their radices in order; entries past n_passes are 0                  */
    int32_t ct_rows;    /* 1: the rows run a kernel with a compile-time plan (four-step M in
                           {250, 1000}, huge M in {10000, 12500}), whose passes take radix 10
                           where it divides, then 5, 3, 8, 4, 2, instead of radix[]; the four-step
                           search (inverse) rows do so only at 25 x 1000 and 16 x 250           */
} gnsship_acq_layout;
int gnsship_acq_layout_get(gnsship_acq* a, gnsship_acq_layout* out);
/* FDMA sweep (GLONASS; pcps_acquisition's is_fdma() / d_doppler_bias, :175-229, :296-301): one code searched
 * under n_channels Doppler grids in one pass.  The wipe-off table holds n_channels × n_bins rows, channel-major;
 * row (g, i) is built from (float)(bias_hz[g] − doppler_max + doppler_center + doppler_step·i), as
 * update_grid_doppler_wipeoffs builds a channel's row with d_doppler_bias = bias_hz[g].  1 ≤ n_channels ≤ 32 (GLONASS
 * has 14) and n_channels·n_bins ≤ 4096, GNSSHIP_E_INVAL otherwise.  n_bins is the ordinary
 * grid's, ceil(2·doppler_max / doppler_step), and what gnsship_acq_num_bins reports.  The buffers that scale with the
 * row count are reallocated when n_channels·n_bins changes.  gnsship_acq_set_grid returns the handle to the ordinary
 * grid; while the FDMA grid is set, gnsship_acq_run and gnsship_acq_set_grid_step2 return GNSSHIP_E_INVAL (two-step
 * acquisition is not available on an FDMA grid). */
int gnsship_acq_set_grid_fdma(gnsship_acq* a, int doppler_max, int doppler_step, int doppler_center, int n_channels, const int32_t* bias_hz);
/* One dwell of the code in prn_slot under every frequency channel of the FDMA grid: the forward transforms and the
 * search run once over all n_channels·n_bins rows; the decision (arg-max, the CFAR opposite-bin row, first against
 * second peak) is taken per channel inside that channel's n_bins rows.  results[n_channels]: doppler_index within the
 * channel, doppler_hz without the bias (as Acq_doppler_hz).  grid (optional, host): n_channels × n_bins × row
 * floats, channel-major.  Non-coherent dwells, bit_transition_flag and zero padding act as in gnsship_acq_run. */
int gnsship_acq_run_fdma(gnsship_acq* a, const void* sig, int fmt, int sig_on_device, int prn_slot, gnsship_acq_result* results, float* grid);
/* Restart the non-coherent dwell accumulation (d_num_noncoherent_integrations_counter = 0 after a
 * decision, pcps_acquisition.cc:783,835,860-864): the next gnsship_acq_run is dwell 1. */
int gnsship_acq_reset_dwells(gnsship_acq* a);
int gnsship_acq_destroy(gnsship_acq* a);

/* Acquisition resampler (GNSS-SDR.use_acquisition_resampler; gnss_flowgraph.cc:1028-1113): the
 * decimating low-pass FIR in front of a channel's acquisition, and the Acq_Conf side
 * (ConfigureAutomaticResampler, acq_conf.cc:91-107).  Taps are GNU Radio's
 * firdes::low_pass(gain, fs, cutoff, transition) with the default Hamming window (GNU Radio is not
 * in the reference tree; restated from its published algorithm). */
typedef struct gnsship_acq_resampler gnsship_acq_resampler;
/* taps == NULL: only *n_taps.  E_INVAL for the arguments firdes rejects (sanity_check_1f). */
int gnsship_firdes_low_pass(double gain, double sampling_freq, double cutoff_freq, double transition_width, float* taps, int taps_cap,
    int* n_taps);
/* The flowgraph's design for a signal whose optimum acquisition rate is opt_acq_fs (e.g.
 * GPS_L1_CA_OPT_ACQ_FS_SPS = 2e6): decimation = floor(fs/opt) lowered until it divides fs, taps =
 * firdes::low_pass(1, fs, fs_dec/2.1, fs_dec/2).  *decimation = 1 and *n_taps = 0 when no resampler
 * is used (opt >= fs or decimation 1).  resampler_latency_samples = (n_taps - 1) / 2. */
int gnsship_acq_resampler_design(int64_t fs_in, double opt_acq_fs, int* decimation, float* taps, int taps_cap, int* n_taps);
/* fir_filter_ccf(decimation, taps) over a sample stream: ntaps - 1 samples of history carried
 * between runs (zeros after create / reset). */
int gnsship_acq_resampler_create(gnsship_ctx* ctx, const float* taps, int n_taps, int decimation, int64_t max_in_samples,
    gnsship_acq_resampler** out);
/* Filter n_in samples (a multiple of the decimation) in `fmt` (converted in the loads, no scaling):
 * n_in / decimation CF32 outputs, left in device memory (*dev_out, valid until the next run) and,
 * when host_out != NULL, copied there before returning.  Asynchronous otherwise (context stream). */
int gnsship_acq_resampler_run(gnsship_acq_resampler* r, const void* in, int fmt, int in_on_device, int64_t n_in, float* host_out,
    void** dev_out, int64_t* n_out);
int gnsship_acq_resampler_reset(gnsship_acq_resampler* r);
int gnsship_acq_resampler_destroy(gnsship_acq_resampler* r);

/* ---------------------------------------------------------------------------------------------
 * Signal conditioner: the frequency-translating FIR decimator the flowgraph puts in front of the
 * channels (Signal_Conditioner, gnss_flowgraph.cc:1008-1140; its InputFilter in the
 * Freq_Xlating_Fir_Filter form, src/algorithms/input_filter/adapters/freq_xlating_fir_filter.cc:36-117,
 * e.g. conf/gnss-sdr_BDS_B3I_GPS_L1_CA_ibyte.conf:41-96).  gr::filter::freq_xlating_fir_filter_ccf(D,
 * taps, fc, fs) restated from its published definition (GNU Radio is not in the reference tree):
 *   y[k] = sum_{i<T} h[i] * x[kD - i] * exp(-j*2*pi*frac(fc*(n0 + kD - i)/fs)),
 * zeros before the stream, n0 = the absolute index of the stream's first sample (0 after create), the
 * fraction exact in integers.  Output k belongs to stream sample kD; the group delay (T - 1)/2 input
 * samples is not compensated, as in the reference.  Fir_Filter is the same stage with if_hz = 0.
 * One handle filters up to GNSSHIP_COND_MAX_BANDS bands of one input stream in one kernel launch per
 * run; the history (max T - 1 samples) and the sample count live on the device, so the same stream cut
 * into runs at any multiples of the decimations gives bit-identical outputs. */
#define GNSSHIP_COND_MAX_BANDS 4
#define GNSSHIP_COND_MAX_TAPS 4096
#define GNSSHIP_COND_MAX_IN_SAMPLES (1LL << 30) /* per run: sizes the launch grid and the handle's output buffers */
typedef struct gnsship_cond gnsship_cond;
/* One band: the adapter's IF, decimation_factor and taps_ (freq_xlating_fir_filter.cc:60-62,96-105). */
typedef struct gnsship_cond_band {
    double if_hz;       /* IF: the band centre moved to 0 [Hz]; a whole number                     */
    int decimation;     /* decimation_factor >= 1                                                  */
    const float* taps;  /* taps_ (copied by create), 1..GNSSHIP_COND_MAX_TAPS of them              */
    int n_taps;
} gnsship_cond_band;
/* The adapter's filter_type=lowpass design (freq_xlating_fir_filter.cc:99-106): firdes::low_pass(1, fs,
 * bw, tw) with bw = 0 -> (fs / decimation) / 2 and tw = 0 -> bw / 10.  Host only; taps == NULL: only
 * *n_taps.  E_INVAL for what firdes rejects. */
int gnsship_cond_lowpass_taps(double fs, int decimation, double bw, double tw, float* taps, int taps_cap, int* n_taps);
/* freq_xlating_fir_filter_ccf::make(decimation, taps, IF, sampling_frequency) (:115) for every band.
 * fs_in (sampling_frequency, :61) a whole number of Hz below 2^31.  E_INVAL (gnsship_last_error says
 * why) for a non-integer fs_in or if_hz, decimation < 1, n_bands outside 1..4, n_taps outside 1..4096,
 * max_in_samples outside 1..GNSSHIP_COND_MAX_IN_SAMPLES or below a band's decimation. */
int gnsship_cond_create(gnsship_ctx* ctx, double fs_in, const gnsship_cond_band* bands, int n_bands, int64_t max_in_samples,
    gnsship_cond** out);
/* Bits per input sample of a format gnsship_cond_run reads: 64 / 32 / 16 (CF32 / CI16 / CI8), 32 / 16 / 8
 * (RF32 / RI16 / RI8), the field width (packed REAL) or twice it (packed IQ / QI); 0 for any other value.
 * Host only. */
int gnsship_cond_fmt_bits(int fmt);
/* The block's work() over n_in samples in `fmt` (converted in the loads, no scaling; the byte / short
 * item types of :118-159 without their converter blocks): n_in / decimation CF32 outputs per band.
 * Real items (GNSSHIP_FMT_RF32 / RI16 / RI8: freq_xlating_fir_filter_fcf / _scf, :118-150) are x with a
 * zero imaginary part; the factor 256 of GNU Radio's char_to_short in front of the byte form (:147), a
 * gain, is not applied.  Packed items (GNSSHIP_FMT_PACKED) are unpacked in the loads; `in` is
 * byte-granular, ceil(n_in * bits / 8) bytes, and sample 0 is field 0 of its first byte.
 * n_in must be a multiple of every band's decimation, of the samples per byte of a packed format,
 * and <= max_in_samples, else E_INVAL and no state changes.  One stream keeps one kind of item (real or
 * complex) between resets: a real run reads only the real part of the carried history.  Band b is written to dev_dst[b] (a caller's device buffer, e.g. a slot of a
 * gnsship_dev_alloc ring) or, where dev_dst or dev_dst[b] is NULL, to the handle's own buffer (valid
 * until the next run); dev_out[b] / n_out[b] (arrays of n_bands, may be NULL) report where and how
 * many.  host_out (may be NULL) / host_out[b] (may be NULL): also copied to the host before returning;
 * asynchronous on the context stream otherwise. */
int gnsship_cond_run(gnsship_cond* c, const void* in, int fmt, int in_on_device, int64_t n_in, void* const* dev_dst,
    float* const* host_out, void** dev_out, int64_t* n_out);
/* Restart the stream (a receiver starting mid-file, as the flowgraph's conditioner starts with the
 * source, gnss_flowgraph.cc:1127-1136): zero history, the next input sample has absolute index
 * first_sample (the phase origin stays at sample 0). */
int gnsship_cond_reset(gnsship_cond* c, uint64_t first_sample);
/* Absolute index of the next input sample (first_sample + everything run since; nitems_read of the
 * block's input). */
int gnsship_cond_samples_in(gnsship_cond* c, uint64_t* n);
int gnsship_cond_destroy(gnsship_cond* c);

/* ---------------------------------------------------------------------------------------------
 * Interference mitigation: the Signal_Conditioner's other InputFilter choices, Pulse_Blanking_Filter,
 * Notch_Filter and Notch_Filter_Lite (src/algorithms/input_filter/adapters/{pulse_blanking_filter,
 * notch_filter,notch_filter_lite}.cc; blocks gnuradio_blocks/{pulse_blanking_cc,notch_cc,notch_lite_cc}.cc).
 * CF32 in, CF32 out.  Each block is defined on the stream, not on the scheduler's buffers: the stream is
 * cut into segments of `length` samples from its first sample, every segment goes through the block's
 * state machine in order, a run emits every complete segment not yet emitted and keeps the rest (and all
 * state) on the device, so the same stream cut into runs anywhere gives bit-identical output and state.
 *   pulse blanking (pulse_blanking_cc.cc:57-98): segment energy E = serial float sum of re*re + im*im;
 *     estimation noise = (float(n)*noise + E/float(2*length))/float(n + 1); blanked when E/noise > thres.
 *   notch (notch_cc.cc:63-121): the block advances its input pointer by one sample without a history
 *     (:72), so output sample k is formed from input sample k + 1 with input sample k as the previous one;
 *     restated as written: segment s is complete once input sample (s + 1)*length has arrived.
 *     out = (x - z0*prev) + (p_c*z0)*last_out, z0 = (cosf(a), sinf(a)), a = atan2f of x*conj(prev) (:95-101).
 *   notch lite (notch_lite_cc.cc:71-138): set_history(2): output k from input k, previous k - 1, zero
 *     before the stream; one z0 per n_segments_coeff segments from the mean of the two end angles (:104-112).
 *   estimation phase of both notches (:77-83 / :85-91): unnormalised forward DFT, VOLK's generic
 *     power spectrum 10*log10f(|X|^2 + 1e-20) and spectral noise floor with the 15 dB exclusion,
 *     pow(10, dB/10)/(2*length).  Not bit-comparable (DFT order); everything else is. */
#define GNSSHIP_MIT_PULSE_BLANKING 0
#define GNSSHIP_MIT_NOTCH 1
#define GNSSHIP_MIT_NOTCH_LITE 2
/* How the notches' one-pole recursion y[n] = b[n] + a[n]*y[n-1] runs on the device; same bits either way.
 * SERIAL: one lane per maximal run of filtered segments.  SPECULATIVE: filtered runs cut into chunks, each
 * started from the zero state warmup_samples early, confirmed bitwise against its predecessor's final
 * state and replayed serially where refuted.  AUTO: see DESIGN.md §8. */
#define GNSSHIP_MIT_CHAIN_AUTO 0
#define GNSSHIP_MIT_CHAIN_SERIAL 1
#define GNSSHIP_MIT_CHAIN_SPECULATIVE 2
#define GNSSHIP_MIT_MAX_LENGTH 1024
#define GNSSHIP_MIT_MAX_IN_SAMPLES (1LL << 30)
typedef struct gnsship_mit gnsship_mit;
/* make_pulse_blanking_cc(pfa, length, n_segments_est, n_segments_reset) (pulse_blanking_cc.cc:26),
 * make_notch_filter(pfa, p_c_factor, length, n_segments_est, n_segments_reset) (notch_cc.cc:25),
 * make_notch_filter_lite(p_c_factor, pfa, length, n_segments_est, n_segments_reset, n_segments_coeff)
 * (notch_lite_cc.cc:26). */
typedef struct gnsship_mit_conf {
    int32_t kind;              /* GNSSHIP_MIT_*                                                      */
    float pfa;                 /* thres_ = upper pfa quantile of chi^2(2*length), unless threshold > 0 */
    float threshold;           /* > 0: thres_ itself, pfa unused; 0: from pfa                        */
    float p_c_factor;          /* notches: pole radius                                               */
    int32_t length;            /* samples per segment, 2..GNSSHIP_MIT_MAX_LENGTH                     */
    int32_t n_segments_est;    /* segments of a noise estimation window, >= 1                        */
    int32_t n_segments_reset;  /* n_segments_ above this restarts the estimate                       */
    int32_t n_segments_coeff;  /* notch lite: segments per z0 update, >= 1                           */
    int32_t chain_form;        /* GNSSHIP_MIT_CHAIN_*                                                */
} gnsship_mit_conf;
typedef struct gnsship_mit_state {
    float noise_power;         /* noise_power_estimation_ / noise_pow_est_                           */
    float threshold;           /* thres_                                                             */
    int32_t n_segments;        /* n_segments_                                                        */
    int32_t n_segments_coeff;  /* n_segments_coeff_ (lite)                                           */
    int32_t filter_state;      /* last_filtered_ / filter_state_                                     */
    int32_t chain_form;        /* the form that runs (AUTO resolved)                                 */
    uint64_t samples_in;       /* since create / reset                                               */
    uint64_t samples_out;
    int64_t pending_samples;   /* arrived, not yet emitted                                           */
    int64_t chunk_samples;     /* speculative form's chunk and warm-up (whole segments)              */
    int64_t warmup_samples;
    uint64_t chunks_speculated; /* chunks started from a predicted state / of those, replayed        */
    uint64_t chunks_replayed;
} gnsship_mit_state;
/* boost::math::quantile(complement(chi_squared(2*length), pfa)) (pulse_blanking_cc.cc:51-52, notch_cc.cc:54-55,
 * notch_lite_cc.cc:63-64), evaluated in double and rounded to float.  Host only.  E_INVAL for pfa outside
 * (0, 1) or length outside 2..1024. */
int gnsship_mit_threshold(double pfa, int length, float* thres);
/* The block's constructor.  E_INVAL (gnsship_last_error says why) for length outside 2..1024, n_segments_est
 * < 1, n_segments_coeff < 1 (lite), pfa outside (0, 1) without a threshold, an unknown kind or chain form,
 * max_in_samples outside 1..GNSSHIP_MIT_MAX_IN_SAMPLES. */
int gnsship_mit_create(gnsship_ctx* ctx, const gnsship_mit_conf* conf, int64_t max_in_samples, gnsship_mit** out);
/* general_work over the next n_in CF32 samples of the stream (0 <= n_in <= max_in_samples, else E_INVAL and
 * no state change).  The complete segments go to dev_dst (a caller's device buffer of at least
 * pending + n_in samples that does not overlap `in`) or, where NULL, to the handle's own buffer (valid until
 * the next run); *dev_out / *n_out (may be NULL) report where and how many samples.  host_out (may be NULL,
 * room for pending + n_in samples): also copied to the host before returning; asynchronous on the context
 * stream otherwise. */
int gnsship_mit_run(gnsship_mit* m, const void* in, int in_on_device, int64_t n_in, void* dev_dst, float* host_out,
    void** dev_out, int64_t* n_out);
/* A fresh block on a fresh stream: the constructor's state, nothing pending. */
int gnsship_mit_reset(gnsship_mit* m);
/* The block's members after everything run so far (waits for the context stream). */
int gnsship_mit_state_get(gnsship_mit* m, gnsship_mit_state* st);
int gnsship_mit_destroy(gnsship_mit* m);

/* ---------------------------------------------------------------------------------------------
 * Viterbi decoding of Galileo pages: the first thing galileo_telemetry_decoder_gs does to an I/NAV, F/NAV or
 * C/NAV page (decode_INAV_word / decode_FNAV_word / decode_CNAV_word, galileo_telemetry_decoder_gs.cc:354-371,
 * :585-599, :684-697): de-interleave (:342-351, out[c*rows + r] = in[r*cols + c]), undo the NOT gate of G2
 * (:362-368, every second de-interleaved symbol negated), Viterbi_Decoder::decode (telemetry_decoder/libs/
 * viterbi_decoder.cc:47-120), here for many channels' frames in one launch, one wavefront per frame.
 * A frame is 2*(data_length + 6) soft symbols as received (interleaved, preamble removed), a one positive.
 *   GNSSHIP_VIT_MODE_REFERENCE reproduces Viterbi_Decoder::decode as written, one object per channel:
 *     1. only the first symbol of each pair enters the metric (:61 copies d_nn - 1 = 1 value, d_rec_array[1]
 *        stays 0): Gamma = {0, 0 + 0, 0 + r0, (0 + 0) + r0} (:151-166);
 *     2. the 64 path metrics carry over from one decode to the next (:56 sets entry 0 alone; -1e7 only in a new
 *        object; reset() does not touch them);
 *     3. d_next_section starts at -1e7, states ascend with a strict > (:70-93): for next state s' the first
 *        predecessor (s' & 31) << 1 wins a tie against the second, and an entry neither lifts above -1e7 is
 *        not stored;
 *     4. the section maximum is subtracted (:96-103); the traceback starts at state 0, skips the 6 tail steps
 *        and emits data_length bits (:107-119).
 *     Bits and carried metrics are bit-equal to the reference's, with one case left out: where the traceback
 *     visits an entry nothing stored in this call, the reference reads what an earlier call left there and this
 *     library reads predecessor 0, bit 0, which is what a new object holds.
 *   GNSSHIP_VIT_MODE_FULL: both symbols in the metric and every frame starts from state 0 alone (the decoder the
 *     code was designed for); the carried metrics are neither read nor written.
 * Inputs are finite by contract; with NaN / Inf the bits are unspecified. */
#define GNSSHIP_VIT_MODE_REFERENCE 0
#define GNSSHIP_VIT_MODE_FULL 1
#define GNSSHIP_VIT_MAX_FRAME_SYMBOLS 1024
#define GNSSHIP_VIT_MAX_CHANNELS (1 << 20)
#define GNSSHIP_VIT_MAX_FRAMES (1 << 22)
typedef struct gnsship_vit gnsship_vit;
typedef struct gnsship_vit_conf {
    int32_t constraint_length;  /* 7; anything else E_INVAL                                          */
    int32_t rate_n;             /* 2; anything else E_INVAL                                          */
    int32_t g[2];               /* generator words, {121, 91} for Galileo; any two 7-bit words       */
    int32_t data_length;        /* LL >= 1; frame = 2*(LL + 6) symbols <= GNSSHIP_VIT_MAX_FRAME_SYMBOLS */
    int32_t interleaver_rows;   /* 0, 0 = none; else rows*cols == 2*(LL + 6)                         */
    int32_t interleaver_cols;
    int32_t invert_g2;          /* != 0: negate every second de-interleaved symbol                   */
    int32_t mode;               /* GNSSHIP_VIT_MODE_*                                                */
} gnsship_vit_conf;
/* One decoder for channels 0..max_channels-1 (1..GNSSHIP_VIT_MAX_CHANNELS), each channel a new
 * Viterbi_Decoder object.  E_INVAL (gnsship_last_error says why) for anything the conf comments exclude. */
int gnsship_vit_create(gnsship_ctx* ctx, const gnsship_vit_conf* conf, int32_t max_channels, gnsship_vit** out);
/* Decode n_frames frames (0..GNSSHIP_VIT_MAX_FRAMES).  symbols: n_frames*frame floats on the host or (on_device)
 * on the device; channels: host int32[n_frames], frame i belongs to channel channels[i]; negate: host
 * uint8[n_frames] or NULL, != 0 negates frame i (d_flag_PLL_180_deg_phase_locked, :1026-1029).  Bits are bytes
 * of 0 / 1, data_length per frame: to bits_dev (a caller's device buffer) or, where NULL, to the handle's own
 * buffer; bits_host (may be NULL): also copied to the host before returning; asynchronous on the context stream
 * otherwise (the host arrays then stay the caller's until the stream has passed the run).  In reference mode a channel's frames are ordered through its carried metrics, so a channel may
 * appear once per call; a duplicate or a channel out of range is E_INVAL and nothing runs.  Full mode checks
 * the channel range only. */
int gnsship_vit_run(gnsship_vit* v, const float* symbols, int on_device, int32_t n_frames, const int32_t* channels,
    const uint8_t* negate, uint8_t* bits_host, void* bits_dev);
/* A new Viterbi_Decoder object on this channel: all 64 metrics -1e7. */
int gnsship_vit_reset_channel(gnsship_vit* v, int32_t channel);
/* d_prev_section of a channel after everything run so far (waits for the context stream). */
int gnsship_vit_state_get(gnsship_vit* v, int32_t channel, float* section /* [64] */);
int gnsship_vit_destroy(gnsship_vit* v);

/* ---------------------------------------------------------------------------------------------
 * Closed-loop tracking engine: the per-epoch DLL/PLL of dll_pll_veml_tracking
 * resident on the device.  Replaces, for N channels at once, the general_work loop of
 * src/algorithms/tracking/gnuradio_blocks/dll_pll_veml_tracking.cc:1728-2094 around
 * do_correlation_step (:1037-1062): cn0_and_tracking_lock_status (:972-1029), run_dll_pll
 * (:1065-1152), update_tracking_vars (:1189-1260), save_correlation_results and the bit /
 * secondary-code synchronisation of states 2 and 4.  start_tracking (:643-883) and the state-1
 * pull-in (:1757-1788) run on the host in gnsship_trk_start.  States 2, 3 (extended coherent
 * integration, extend_correlation_symbols > 1) and 4, with the FLL branches (enable_fll_*) and
 * high_dyn (high-dynamics correlator fed by the smoothed NCO rates); BeiDou B1I GEO satellites by
 * the start arguments' PRN.
 * ------------------------------------------------------------------------------------------- */
#define GNSSHIP_SYS_GPS_L1CA 0 /* GPS L1 C/A: 3 taps, bit sync on the 160-symbol preamble */
#define GNSSHIP_SYS_GAL_E1 1   /* Galileo E1 B/C: VEML 5 taps on the pilot + data prompt, CS25 secondary */
#define GNSSHIP_SYS_BDS_B1I 2  /* BeiDou B1I MEO/IGSO (PRN 6-58): 3 taps, 20-chip NH secondary code */
/* GPS L5 (dll_pll_veml_tracking.cc:213-247, gps_l5_dll_pll_tracking.cc:44-65): 3 taps on the L5Q pilot
 * (NH20 secondary code) + the L5I data prompt (NH10, 10 symbols per bit).  track_pilot must be 1:
 * data-only tracking (the reference's d_interchange_iq) is not restated and gnsship_trk_create
 * rejects it with GNSSHIP_E_INVAL.  slope, spc and y_intercept are set as the block sets them
 * (1, early_late_space_chips, 1), whatever the configuration carries. */
#define GNSSHIP_SYS_GPS_L5 3
/* BeiDou B3I (dll_pll_veml_tracking.cc:415-434, :799-834; Beidou_B3I.h): 3 taps, no pilot (track_pilot is forced
 * to 0).  MEO/IGSO satellites carry the 20-chip NH secondary code (20 symbols per bit); GEO satellites — start's
 * prn in 1..5 or > 58, as B1I — 2 symbols per bit, no NH, the D2 preamble as synchronisation pattern and
 * extend_correlation_symbols capped at 2.  extend_correlation_symbols is clamped to [1, 20]. */
#define GNSSHIP_SYS_BDS_B3I 4
/* GPS L2C, the L2 CM code (:196-212, :666-668; gps_l2_m_dll_pll_tracking.cc:44-62): 3 taps, one 20 ms code period
 * per telemetry symbol (vector_length = fs / 50, the loop filters updated every 20 ms), no secondary code, no
 * pilot: track_pilot is forced to 0 and extend_correlation_symbols to 1. */
#define GNSSHIP_SYS_GPS_L2C 5
/* Galileo E5a ("5X", dll_pll_veml_tracking.cc:292-322, :699-722; galileo_e5a_dll_pll_tracking.cc:47-58) and E5b
 * ("7X", :323-353, :723-746): 10230 chips at 10.23 Mcps, 1 ms, 3 taps; slope, spc and y_intercept set as the block
 * sets them (1, early_late_space_chips, 1); extend_correlation_symbols raised to 1 at least.
 *   track_pilot = 1: 3 taps on the Q primary (start's code_id) + the I primary on the data prompt (data_code_id) —
 *     the GPS L5 layout.  The pilot's 100-chip secondary code belongs to the satellite: start's prn selects it
 *     (E5a: 1..47, E5b: 1..50; GNSSHIP_E_INVAL otherwise).  The I secondary code (E5a 20 chips / 20 symbols per bit,
 *     E5b 4 / 4) is stripped from the data prompt.  d_interchange_iq (:313, :344, :1945-1949, :1997-2001): the
 *     valid-symbol prompt_i / prompt_q of gnsship_trk_epoch are the data prompt's imaginary / real part; dump
 *     records (log_data) are not exchanged.
 *   track_pilot = 0: 3 taps on the I primary, no data prompt — the BeiDou B3I layout; the I secondary code is the
 *     synchronisation pattern and is removed from the taps, the symbol prompt sums the epochs' own prompts over
 *     symbols-per-bit epochs (d_data_secondary_code_length stays 0), no exchange, and extend_correlation_symbols is
 *     capped at the I secondary length (20 / 4).  start's prn must be in 1..50. */
#define GNSSHIP_SYS_GAL_E5A 6
#define GNSSHIP_SYS_GAL_E5B 7
/* GLONASS L1 / L2 C/A: not dll_pll_veml_tracking but glonass_l1_ca_dll_pll_tracking_cc (glonass_l2_…: the same block with
 * the L2 constants) — 3 taps at ∓early_late_space_chips, two second-order float loop filters (Tracking_2nd_DLL_filter,
 * Tracking_2nd_PLL_filter: ζ 0.7, pdi 1 ms, coefficients fixed at create from dll_bw_hz / pll_bw_hz), no bit or secondary
 * synchronisation states, a lock test every CN0_ESTIMATION_SAMPLES + 1 = 11 epochs.  The carrier NCO carries the channel's
 * FDMA offset DFRQ·k, k from start's PRN through gnsship_glonass_freq_channel (GNSSHIP_E_INVAL for a PRN outside the
 * table); carrier_doppler_hz is reported without it.  Of gnsship_trk_conf the block reads fs_in, vector_length
 * (round(fs / 1000)), pll_bw_hz, dll_bw_hz, early_late_space_chips, carrier_lock_th, cn0_min, max_carrier_lock_fail (the
 * block's gflags carrier_lock_th / cn0_min / max_lock_fail), if_hz and rotator; cn0_samples only sizes the prompt buffer
 * (the test length is 10).  Ignored: track_pilot, the FLL fields, the narrow spacings and bandwidths,
 * very_early_late_space_chips, extend_correlation_symbols, high_dyn, the smoothers, slope / spc / y_intercept,
 * max_code_lock_fail, pull_in_time_s, bit_synchronization_time_limit_s, carrier_aiding and the filter orders.  rotator must
 * be GNSSHIP_ROTATOR_GENERIC (create: GNSSHIP_E_INVAL otherwise — the SIMD forms of the complex-code rotator are not
 * restated).  The loop runs on the persistent generic pipeline only (gnsship_trk_last_engine: _PERSIST); a run that cannot
 * use it returns GNSSHIP_E_INVAL.  Records: state 4; flags 8 every epoch, 1 Flag_valid_symbol_output, 2 on loss of lock (the
 * channel stops), 16 with dump; prompt_i / prompt_q the epoch's prompt on every epoch; sample_counter the epoch's first
 * sample.  The epoch is correlated over the block length the previous epoch left and consumes the new one, as the block
 * does.  Dump records (:641-701): PRN_start_sample_count is the epoch's first sample, both rate fields 0. */
#define GNSSHIP_SYS_GLO_L1CA 8
#define GNSSHIP_SYS_GLO_L2CA 9

typedef struct gnsship_trk_conf { /* Dll_Pll_Conf (dll_pll_conf.h:33-80), same names and units */
    double fs_in;
    double carrier_lock_th;
    float pll_bw_hz;
    float dll_bw_hz;
    float fll_bw_hz;
    float early_late_space_chips;
    float very_early_late_space_chips;
    float slope;
    float spc;
    float y_intercept;
    float cn0_smoother_alpha;
    float carrier_lock_test_smoother_alpha;
    uint32_t pull_in_time_s;
    uint32_t bit_synchronization_time_limit_s;
    uint32_t vector_length;
    int32_t pll_filter_order;
    int32_t dll_filter_order;
    int32_t cn0_samples;
    int32_t cn0_smoother_samples;
    int32_t carrier_lock_test_smoother_samples;
    int32_t cn0_min;
    int32_t max_code_lock_fail;
    int32_t max_carrier_lock_fail;
    int32_t carrier_aiding;
    int32_t track_pilot;
    int32_t system; /* GNSSHIP_SYS_*: the signal constants the adapter selects */
    int32_t extend_correlation_symbols; /* > 1: extended coherent integration, state 3 (:515-523) */
    float pll_bw_narrow_hz;
    float dll_bw_narrow_hz;
    float early_late_space_narrow_chips;
    float very_early_late_space_narrow_chips;
    int32_t enable_fll_pull_in;      /* FLL-assisted carrier loop during the pull-in (:1080-1097) */
    int32_t enable_fll_steady_state; /* ... and after it */
    int32_t high_dyn;                /* high-dynamics correlator + NCO rate smoothing (:1205-1255) */
    uint32_t smoother_length;        /* rate smoother length, 1..64 (0 is raised to 1, dll_pll_conf.cc:118-123) */
    int32_t rotator;                 /* GNSSHIP_ROTATOR_*: which volk_gnsssdr rotator variant the correlations
                                        reproduce (0 = generic; high_dyn has only the generic variant) */
    int32_t reserved0;               /* 0 */
    /* ABI 2.  Carrier IF of this engine's signal in the IF buffer [Hz] (e.g. +7.161e6 for GPS L1 / Galileo
     * E1 and −7.161e6 for BeiDou B1I in a 1568.259 MHz-centred front end).  The reference removes it
     * ahead of the channels (InputFilter.IF → freq_xlating_fir_filter, conf/gnss-sdr_BDS_B3I_GPS_L1_CA_
     * ibyte.conf:45-92; GNSSFlowgraph connects the filtered output to every channel); here it is fused
     * into the correlator's carrier NCO: phase_step = (float)(carrier_phase_step_rad + 2π·if_hz/fs) and
     * rem_carrier_phase = (float)fmod(rem_carr_phase_rad + 2π·frac(if_hz·n/fs), 2π) at the epoch's first
     * absolute sample n (frac(if_hz·n/fs) carried per channel in double, exact for integer if_hz and
     * fs).  The loop, its Doppler, carrier phase and all outputs stay IF-free, as in the reference.
     * 0 = the buffer is at baseband. */
    double if_hz;
} gnsship_trk_conf;

typedef struct gnsship_trk_start_args { /* Gnss_Synchro fields start_tracking reads (:647-649) */
    int32_t code_id;      /* code-bank entry of the tracking replica (pilot for E1) */
    int32_t data_code_id; /* E1 / E5a / E5b with track_pilot and GPS L5: data replica (E1-B / E5a-I / E5b-I / L5I); otherwise ignored */
    double acq_delay_samples;
    double acq_doppler_hz;
    uint64_t acq_samplestamp_samples;
    uint64_t first_sample; /* nitems_read when the block first runs after start (state-1 pull-in) */
    int32_t prn;           /* Gnss_Synchro::PRN: BeiDou B1I PRN 1-5 and 59+ are GEO satellites (:765-781);
                              Galileo E5a / E5b: selects the pilot's secondary code (:706, :730) */
    int32_t reserved;      /* 0 */
} gnsship_trk_start_args;

typedef struct gnsship_trk_epoch { /* one general_work call of one channel (Gnss_Synchro subset) */
    uint64_t sample_counter;       /* nitems_read at the epoch start */
    double prompt_i, prompt_q;     /* valid when flags & 1 (state 4 symbol output); E5a / E5b with track_pilot: exchanged */
    double code_phase_samples;     /* d_rem_code_phase_samples */
    double carrier_phase_rads;     /* d_acc_carrier_phase_rad */
    double carrier_doppler_hz;
    double cn0_db_hz;
    float carrier_lock_test;
    int32_t state;                 /* state the epoch ran in (2, 3 or 4) */
    int32_t flags;                 /* 1 valid symbol, 2 loss of lock, 4 PLL 180°, 8 epoch ran,
                                      16 log_data record written (gnsship_trk_run_dump) */
    int32_t pad;
    double code_freq_chips;
    double rem_code_phase_chips;
    float rem_carr_phase_rad;
    int32_t prn_length_samples;    /* d_current_prn_length_samples after the update */
} gnsship_trk_epoch; /* 96 bytes */

typedef struct gnsship_trk gnsship_trk;
int gnsship_trk_create(gnsship_ctx* ctx, const gnsship_trk_conf* conf, int max_channels, gnsship_trk** out);
int gnsship_trk_start(gnsship_trk* t, int channel, const gnsship_trk_start_args* args);
/* n gnsship_trk_start calls in one transaction (a mass hand-off from acquisition): channels[i]
 * starts from args[i]; every channel is validated before any device state changes (on an error
 * nothing is started); one upload, one scatter launch, one synchronisation.  Distinct channels. */
int gnsship_trk_start_many(gnsship_trk* t, int n, const int32_t* channels, const gnsship_trk_start_args* args);
int gnsship_trk_stop(gnsship_trk* t, int channel);
/* msg_handler_telemetry_to_trk (dll_pll_veml_tracking.cc:617-640): a telemetry fault (tlm_event 1)
 * from the channel's telemetry decoder sets the carrier lock-fail counter to 200000, so the next
 * lock check of the loop declares loss of lock.  Other event values are ignored, as there. */
int gnsship_trk_telemetry_event(gnsship_trk* t, int channel, int tlm_event);
/* Runs up to max_rounds epochs of every tracking channel over the IF buffer holding absolute
 * samples [buffer_first_sample, +n_buffer_samples) (device pointer when sig_on_device, else host
 * memory staged to the device).  Per round each channel whose next vector_length window lies in
 * the buffer runs one epoch; no host round trip between rounds.  out (optional): max_rounds ×
 * max_channels records, flags & 8 marking the epochs that ran.  *rounds_done: rounds in which at
 * least one channel ran. */
int gnsship_trk_run(gnsship_trk* t, const void* sig, int fmt, int sig_on_device, uint64_t buffer_first_sample, int64_t n_buffer_samples,
    int max_rounds, gnsship_trk_epoch* out, int* rounds_done);
/* The tracking dump record dll_pll_veml_tracking::log_data writes per valid loop update when
 * `dump` is on (:1376-1466; read back by tracking_dump_reader.cc:26-47): 96 bytes, packed exactly
 * as the file — a per-channel .dat dump is the concatenation of the records whose epoch has
 * flags & 16, in round order. */
#pragma pack(push, 4)
typedef struct gnsship_trk_dump_record {
    float abs_VE, abs_E, abs_P, abs_L, abs_VL; /* |accumulators| (VE/VL 0 without VEML)            */
    float prompt_I, prompt_Q;                 /* this epoch's prompt (data prompt with track_pilot) */
    uint64_t PRN_start_sample_count;          /* nitems_read + d_current_prn_length_samples     */
    float acc_carrier_phase_rad;
    float carrier_doppler_hz;
    float carrier_doppler_rate_hz;            /* carrier_phase_rate_step_rad·fs²/2π (high_dyn)   */
    float code_freq_chips;
    float code_freq_rate_chips;               /* code_phase_rate_step_chips·fs²                  */
    float carr_error_hz, carr_error_filt_hz;
    float code_error_chips, code_error_filt_chips;
    float CN0_SNV_dB_Hz, carrier_lock_test;
    float aux1;                               /* d_rem_code_phase_samples                        */
    double aux2;                              /* (double)(nitems_read + prn length)              */
    uint32_t PRN;
} gnsship_trk_dump_record;
#pragma pack(pop)
/* gnsship_trk_run that also fills dump[max_rounds × max_channels] (optional) with the log_data
 * records of the epochs flagged 16. */
int gnsship_trk_run_dump(gnsship_trk* t, const void* sig, int fmt, int sig_on_device, uint64_t buffer_first_sample, int64_t n_buffer_samples,
    int max_rounds, gnsship_trk_epoch* out, gnsship_trk_dump_record* dump, int* rounds_done);
/* Asynchronous form: enqueue the run on the context stream and return (dev_sig: a device buffer that
 * stays valid until gnsship_trk_collect); records / dump records are kept on the device when
 * requested.  Engines on different contexts of one device then run concurrently from one host
 * thread (e.g. a hybrid receiver's GPS, Galileo and BeiDou engines over one IF block).  Every launch
 * is followed by exactly one gnsship_trk_collect, which waits for it and copies the records
 * (out / dump as in gnsship_trk_run_dump, NULL to skip; a non-NULL out / dump that the launch did not
 * keep — want_records / want_dump 0 — is GNSSHIP_E_INVAL, the buffer untouched, the launch finished). */
int gnsship_trk_launch(gnsship_trk* t, const void* dev_sig, int fmt, uint64_t buffer_first_sample, int64_t n_buffer_samples, int max_rounds,
    int want_records, int want_dump);
int gnsship_trk_collect(gnsship_trk* t, gnsship_trk_epoch* out, gnsship_trk_dump_record* dump, int* rounds_done);
/* Where the last gnsship_trk_run / _launch that kept records left them on the device: rounds × max_channels records,
 * round-major, written in context-stream order (valid until the handle's next run or its destruction; before or after
 * gnsship_trk_collect).  A query only.  GNSSHIP_E_STATE when the last run kept none. */
int gnsship_trk_records_device(gnsship_trk* t, const gnsship_trk_epoch** dev_ptr, int32_t* rounds, int32_t* max_channels);
int gnsship_trk_channel_state(gnsship_trk* t, int channel, int* state, uint64_t* next_sample);
/* Correlation trace: each channel-epoch's do_correlation_step call (dll_pll_veml_tracking.cc:1037-1062)
 * as the engine ran it — the float arguments of Carrier_wipeoff_multicorrelator_resampler
 * (cpu_multicorrelator_real_codes.cc:103-126, the carrier ones with the IF folded in) and the
 * correlator outputs — so that a caller can re-run exactly those correlations on the reference's
 * CPU correlator and compare them tap by tap.  Off by default (a debugging aid: 104 bytes per
 * channel-epoch written to HBM). */
typedef struct gnsship_trk_corr_trace {
    uint64_t sample_counter;               /* absolute first sample of the epoch (nitems_read) */
    int32_t n_samples;                     /* vector_length */
    int32_t n_taps;
    float rem_carrier_phase_rad, phase_step_rad;
    float rem_code_phase_samples, code_phase_step_samples;  /* rem_code_phase_chips·spc, code_phase_step_chips·spc */
    float shifts[5];                       /* local code shifts in code samples (narrow taps once narrowed) */
    float taps[10];                        /* complex output per tap */
    float data_prompt[2];                  /* the data correlator's prompt (track_pilot), else 0 */
    int32_t pad;
} gnsship_trk_corr_trace; /* 104 bytes */
int gnsship_trk_set_trace(gnsship_trk* t, int enable);
/* The last run's trace: max_rounds × max_channels records (the run's max_rounds), zero where no epoch ran. */
int gnsship_trk_trace_records(gnsship_trk* t, gnsship_trk_corr_trace* out, int max_records);
/* Which kernel the last gnsship_trk_run / _launch ran (GNSSHIP_TRK_ENGINE_*; NONE before any run):
 * the AVX rotator runs trk_fast's latency form while the channels fit one per compute unit and
 * trk_lane beyond (one 16-lane row per channel; trk_fast's throughput form when a code is not ±1),
 * the generic rotator trk_persist, high_dyn and epochs too long for LDS the round-based loop. */
#define GNSSHIP_TRK_ENGINE_NONE 0
#define GNSSHIP_TRK_ENGINE_FAST_LATENCY 1
#define GNSSHIP_TRK_ENGINE_FAST_THROUGHPUT 2
#define GNSSHIP_TRK_ENGINE_PERSIST 3
#define GNSSHIP_TRK_ENGINE_ROUNDS 4
#define GNSSHIP_TRK_ENGINE_LANES 5
int gnsship_trk_last_engine(gnsship_trk* t, int* engine);
/* What the last gnsship_trk_run / _launch decided beyond the engine: the kernel variant and its LDS plan, as the
 * launch function chose them (a member that does not apply to the engine is 0; everything but `engine` and `format`
 * is 0 for _ROUNDS and _NONE).  A query only: it changes nothing and reads no environment variable. */
typedef struct gnsship_trk_plan {
    int32_t engine;       /* GNSSHIP_TRK_ENGINE_* (what gnsship_trk_last_engine returns) */
    int32_t format;       /* GNSSHIP_FMT_* of the run's samples */
    int32_t n_taps;       /* 3 or 5 */
    int32_t data_prompt;  /* 1: a second replica for the data prompt (track_pilot) */
    int32_t packed;       /* trk_fast: the replicas held as sign bits (trk_lane always holds them so: 0 there) */
    int32_t sring;        /* trk_fast: the phasor slots in a ring (rs tasks) instead of one per task of the epoch */
    int32_t rs, rg;       /* trk_fast: phasor slots (tasks) and product groups held in LDS */
    int32_t lds_bytes;    /* dynamic LDS of the launch */
    int32_t thru;         /* trk_fast: the throughput form (3-tap layouts only); trk_persist: the variant at 4 waves per SIMD */
    int32_t long_plan;    /* trk_fast's latency form: the wave-role plan of long epochs (vector_length >= 10000) */
    int32_t avx;          /* trk_persist: the AVX rotator's form, u_avx's sixteen chains on sixteen lanes (else the generic serial pipeline) */
    int32_t lane_waves;   /* trk_lane: waves per workgroup (4 channels each) */
    int32_t reserved[3];
} gnsship_trk_plan; /* 64 bytes */
int gnsship_trk_last_plan(gnsship_trk* t, gnsship_trk_plan* plan);
int gnsship_trk_destroy(gnsship_trk* t);

/* ---------------------------------------------------------------------------------------------
 * Galileo telemetry framing on the device: the frame handling of galileo_telemetry_decoder_gs::general_work
 * (galileo_telemetry_decoder_gs.cc:872-1094) for I/NAV (E1-B, E5b-I), F/NAV (E5a-I) and C/NAV frame geometry, one
 * block object per channel, one wavefront per channel.  Per symbol, in the block's order: push_back into the symbol
 * history (capacity required + 1, :884), d_symbol_counter++ (:886), check_tlm_separation (:856-869), then the switch on
 * d_stat: states 0 / 1 correlate the P oldest history entries with the preamble once the history is full (an entry is
 * negative only when `< 0.0`; |corr| >= P is a hit; state 1 accepts a hit exactly one period after the last, falls back
 * to 0 on a later one and ignores an earlier one), state 2 decodes when counter == preamble_index + period: the frame is
 * history[P .. P + frame), negated under the 180° flag, de-interleaved, G2-flipped and Viterbi-decoded as gnsship_vit
 * does (same modes, the carried metrics per channel), then the page handling of decode_INAV/FNAV/CNAV_word up to the
 * CRC and the CRC-error counter (more than 6 consecutive failures: loss of sync, back to state 0).
 *   geometry        preamble          P   period  required  frame  rows x cols   LL   fault after
 *   I/NAV           0101100000        10   250     510       240    8 x 30       114  15000 symbols
 *   F/NAV           101101110000      12   500     512       488    8 x 61       238   2500
 *   C/NAV           1011011101110000  16  1000    1016       984    8 x 123      486  60000
 * I/NAV: an even part (first bit 0) is stored and tests nothing; an odd part joins the stored even part, CRC-24Q over
 * bits [0, 196) of the joined string against [196, 220), and clears the stored flag; an odd part with no stored even
 * part tests nothing.  flag_CRC_test is sticky (written only at a joined odd part, cleared by nothing), so crc_ok after
 * an even part is the previous odd part's verdict and the first part after sync counts as an error — as the block.
 * F/NAV: CRC over [0, 214) against [214, 238), C/NAV: [0, 462) against [462, 486), on every page.  The block decodes a
 * C/NAV page only when the symbol's sampling rate is non-zero (:1040); here it is taken as non-zero always.
 * A page part is emitted required + 1 + 2*period symbols after its preamble's first symbol at the earliest: the
 * correlation looks at the oldest end of a full history.
 * Not here: TOW and everything below :1096, page_jk_decoder / ephemeris fields, Reed-Solomon, HAS header parsing and the
 * dummy-page test, time tags, the nav-data monitor, the CRC statistics file, the .dat dump, other systems' telemetry (GPS L1 C/A LNAV: gnsship_lnav_*, GPS CNAV: gnsship_cnav_*, BeiDou D1/D2: gnsship_dnav_*, all below).
 * Symbols are finite by contract; with NaN / Inf the decoded bits are unspecified (nothing is read or written out of
 * bounds: every index comes from lane numbers, sizes and ballot bits). */
#define GNSSHIP_TLM_INAV 1
#define GNSSHIP_TLM_FNAV 2
#define GNSSHIP_TLM_CNAV 3
#define GNSSHIP_TLM_MAX_CHANNELS (1 << 20)
#define GNSSHIP_TLM_MAX_ROUNDS (1 << 20)
typedef struct gnsship_tlm gnsship_tlm;
typedef struct gnsship_tlm_conf {
    int32_t frame_type;      /* GNSSHIP_TLM_*                                                  */
    int32_t vit_mode;        /* GNSSHIP_VIT_MODE_REFERENCE (default, parity) or _FULL          */
    int32_t max_rounds;      /* most symbols per channel in one run, >= 1                      */
    int32_t reserved;        /* 0 */
} gnsship_tlm_conf;
typedef struct gnsship_tlm_page {   /* one decoded page part, 32 bytes */
    uint64_t symbol_counter;        /* d_symbol_counter at the part's last symbol              */
    uint64_t sample_counter;        /* the completing epoch's record.sample_counter; 0 for run_symbols */
    int32_t channel;
    int32_t flags;                  /* 1 crc_ok as the block computes it (sticky for I/NAV), 2 a CRC was evaluated on
                                       this part, 4 PLL 180°, 8 I/NAV odd part, 16 frame sync after this part,
                                       32 sync lost at this part (d_stat back to 0)            */
    int32_t crc_error_counter;      /* after this part */
    int32_t pad;
} gnsship_tlm_page;
typedef struct gnsship_tlm_state { /* the block's members, for tests and diagnosis */
    uint64_t symbol_counter, preamble_index, last_valid_preamble;
    int32_t stat, crc_error_counter, history_size;
    uint8_t pll_180, frame_sync, even_word_arrived, flag_crc_test, sent_tlm_failed, pad[3];
} gnsship_tlm_state;
/* Channels 0..max_channels-1 (1..GNSSHIP_TLM_MAX_CHANNELS), each a new block object: empty history, counters 0,
 * d_stat 0, all 64 Viterbi metrics -1e7.  A run emits at most pages_per_run = max_rounds / period + 1 parts per
 * channel.  Device memory per channel: the history ring (required + 1 floats: 2 KiB I/NAV, 4 KiB C/NAV), 64 bytes of
 * members, 256 of metrics, and pages_per_run slots of 32 + LL bytes. */
int gnsship_tlm_create(gnsship_ctx* ctx, const gnsship_tlm_conf* conf, int32_t max_channels, gnsship_tlm** out);
/* symbols[r*max_channels + c], r < n_rounds (0..max_rounds), float on the host or (on_device) on the device; valid:
 * uint8 of the same shape and place, or NULL for all valid.  Channel c consumes its valid entries in order of r.
 * Outputs, in the handle's own device buffers (gnsship_tlm_outputs_device) and copied to whichever host pointers are
 * given: pages[c][k] and bits[c][k][LL] (bytes of 0 / 1) for k < counts[c], the parts channel c emitted in this run in
 * order (slots beyond counts[c] are unspecified); counts int32[c]; faults uint8[c], 1 where check_tlm_separation fired
 * in this run.  With no host pointer the call is asynchronous on the context stream (host inputs then stay the
 * caller's until the stream has passed the run). */
int gnsship_tlm_run_symbols(gnsship_tlm* t, const float* symbols, const uint8_t* valid, int on_device, int32_t n_rounds,
    gnsship_tlm_page* pages_host, uint8_t* bits_host, int32_t* counts_host, uint8_t* faults_host);
/* The same over tracking records of that shape: an entry is a symbol when flags & 1, the symbol is (float)prompt_i
 * (as :884 narrows the double), the page's sample_counter the completing record's. */
int gnsship_tlm_run_records(gnsship_tlm* t, const gnsship_trk_epoch* records, int on_device, int32_t n_rounds,
    gnsship_tlm_page* pages_host, uint8_t* bits_host, int32_t* counts_host, uint8_t* faults_host);
/* The same over the records the tracker's last run left on the device (gnsship_trk_records_device), in place, ordered
 * on the context stream; before or after gnsship_trk_collect.  E_STATE if there are none; E_INVAL if the handles are
 * on different contexts, their max_channels differ or the run had more rounds than max_rounds. */
int gnsship_tlm_run_trk(gnsship_tlm* t, gnsship_trk* trk, gnsship_tlm_page* pages_host, uint8_t* bits_host, int32_t* counts_host,
    uint8_t* faults_host);
/* The handle's output buffers (any pointer may be NULL) and pages_per_run. */
int gnsship_tlm_outputs_device(gnsship_tlm* t, gnsship_tlm_page** pages, uint8_t** bits, int32_t** counts, uint8_t** faults,
    int32_t* pages_per_run);
/* The block's reset() (:792-820): d_flag_frame_sync false, d_stat 0, d_last_valid_preamble = d_symbol_counter, the
 * fault flag cleared.  History, counters, 180° flag, the stored even part, flag_CRC_test and the Viterbi metrics stay. */
int gnsship_tlm_reset_channel(gnsship_tlm* t, int32_t channel);
/* set_satellite() (:771-789): d_last_valid_preamble = d_symbol_counter, the fault flag cleared. */
int gnsship_tlm_set_satellite(gnsship_tlm* t, int32_t channel);
/* A new block object on this channel. */
int gnsship_tlm_new_channel(gnsship_tlm* t, int32_t channel);
/* The channel's members after everything run so far (waits for the context stream). */
int gnsship_tlm_state_get(gnsship_tlm* t, int32_t channel, gnsship_tlm_state* st);
int gnsship_tlm_destroy(gnsship_tlm* t);

/* ---------------------------------------------------------------------------------------------
 * GPS L1 C/A telemetry on the device: gps_l1_ca_telemetry_decoder_gs (gps_l1_ca_telemetry_decoder_gs.cc) up to the
 * time of week, one block object per channel, one wavefront per channel, no float arithmetic.  Per symbol, in the
 * block's order (general_work, :564-707):
 *   seeding     an empty history (a new object, or after reset) first receives the 8 preamble values 10001011 ('1' -> +1,
 *               '0' -> -1), negated when the incoming symbol carries the 180° flag, and the counter grows by 8 (:573-590).
 *   push        (float)Prompt_I into a history of capacity 300, counter++, d_flag_preamble = false.
 *   separation  check_tlm_separation (:448-460) fires once, until reset, when counter - last_valid_preamble > 6000.
 *   state 0     on a full history the 8 oldest entries are correlated with the preamble (an entry is negative only when
 *               `< 0.0`); |corr| >= 8 is a hit: preamble_index = counter, the 180° flag becomes corr < 0 and stays so
 *               even if the decode fails, d_prev_GPS_frame_4bytes = 0, decode_subframe.  On success the error counter is
 *               0, last_valid_preamble = counter, frame sync, state 1.  Hit or not, state 0 ends with flag_TOW_set false.
 *   state 1     when counter >= preamble_index + 300: preamble_index = counter and decode under the stored 180° flag; the
 *               previous word is NOT cleared, it carries over from the last decode, failed or not.  A failure counts; more
 *               than 2 in a row: frame sync false, state 0, both TOW members 0, the error counter 0, flag_TOW_set false.
 *   decode      (:261-433) over the 300 entries, oldest first: a bit is 1 when the symbol is > 0 (inverted: < 0), so a
 *               zero, a -0 or a NaN is a 0 bit under both polarities and counts as positive in the correlation — exactly,
 *               this is part of the contract.  Every 30 bits: bits 30 / 31 of the word are bits 0 / 1 of the previous word
 *               as stored; with bit 30 set the word is XORed with 0x3FFFFFC0; the parity check of :191-214; the word
 *               becomes the previous word.  Any failing word fails the subframe but all ten are processed.  After ten
 *               good parities the subframe ID is (word2 >> 8) & 7; for 1..5 the navigation object's TOW becomes
 *               6 * ((word2 >> 13) & 0x1FFFF) (gps_navigation_message.cc:98-273) and the decode returns true; any other
 *               ID leaves the TOW alone and the decode returns false.
 *   stamp       (:605-629) a valid subframe with a non-zero navigation TOW sets both TOW members to TOW * 1000 and
 *               flag_TOW_set; with a zero TOW nothing happens, not even the increment (a stale value may be output);
 *               any other symbol adds 20 ms if flag_TOW_set.  The block outputs the symbol only when flag_TOW_set.
 * Not here: ephemeris, iono, UTC and almanac fields and their messages, hybrid mode, the nav-data monitor, the CRC
 * statistics file, dumps, time tags, and the pi added to the carrier phase (the 180° flag is in the output instead). */
#define GNSSHIP_LNAV_MAX_CHANNELS (1 << 20)
#define GNSSHIP_LNAV_MAX_ROUNDS (1 << 20)
/* The most records one run of max_rounds symbols can emit.  Every record sets preamble_index, so the next state-1 decode
 * is 300 symbols later: consecutive records are >= 300 symbols apart, except a state-0 success, which may follow a loss
 * of sync by one symbol.  A loss needs three consecutive state-1 failures after the last success (the first loss of a
 * run may find the error counter at 2 already), so losses are >= 901 symbols apart: with L losses in n symbols,
 * n >= 1 + 300 (R - 1 - L) + L and L <= (n - 1) / 901 + 1, hence R <= n / 300 + n / 900 + 2.  (n / 300 + 2 holds for
 * n < 900 only: 1, 2, 302, 602, 902, 903 are six records in 903 symbols.) */
#define GNSSHIP_LNAV_SUBFRAMES_PER_RUN(max_rounds) ((max_rounds) / 300 + (max_rounds) / 900 + 2)
typedef struct gnsship_lnav gnsship_lnav;
typedef struct gnsship_lnav_conf {
    int32_t max_rounds;      /* most entries per channel in one run, >= 1 */
    int32_t reserved;        /* 0 */
} gnsship_lnav_conf;
typedef struct gnsship_lnav_subframe { /* one decode_subframe call that was emitted, 80 bytes */
    uint64_t symbol_counter;        /* d_sample_counter at the subframe's last symbol */
    uint64_t sample_counter;        /* the completing epoch's record.sample_counter; 0 for run_symbols */
    uint32_t words[10];             /* as the block stores them: data bits un-inverted, bits 30 / 31 = D30* / D29* */
    int32_t channel;
    int32_t subframe_id;            /* (words[1] >> 8) & 7, whatever the parities */
    uint32_t tow_s;                 /* the navigation object's TOW after this decode */
    int32_t crc_error_counter;      /* after this decode */
    uint32_t parity_fail_mask;      /* bit i: word i failed */
    int32_t flags;                  /* 1 decode_subframe returned true, 2 all ten parities passed, 4 PLL 180°,
                                       8 decoded in state 1, 16 frame sync after it, 32 sync lost here */
} gnsship_lnav_subframe;
#ifdef __cplusplus
static_assert(sizeof(gnsship_lnav_subframe) == 80, "gnsship_lnav_subframe");
#else
_Static_assert(sizeof(gnsship_lnav_subframe) == 80, "gnsship_lnav_subframe");
#endif
typedef struct gnsship_lnav_state { /* the block's members, for tests and diagnosis, 64 bytes */
    uint64_t symbol_counter, preamble_index, last_valid_preamble;
    uint64_t subframes_tried;       /* a diagnostic: every decode_subframe call, failed state-0 attempts included */
    uint32_t prev_word;             /* d_prev_GPS_frame_4bytes */
    uint32_t tow_at_preamble_ms, tow_at_current_symbol_ms;
    uint32_t nav_tow_s;             /* d_nav.get_TOW() */
    int32_t stat, crc_error_counter, history_size;
    uint8_t pll_180, frame_sync, tow_set, sent_tlm_failed;
} gnsship_lnav_state;
/* sflags of an entry */
#define GNSSHIP_LNAV_S_OUTPUT 1     /* the block output this symbol (flag_TOW_set) */
#define GNSSHIP_LNAV_S_PLL_180 2    /* d_flag_PLL_180_deg_phase_locked after this symbol */
#define GNSSHIP_LNAV_S_SUBFRAME 4   /* this symbol completed a valid subframe (d_flag_preamble) */
/* Channels 0..max_channels-1 (1..GNSSHIP_LNAV_MAX_CHANNELS), each a new block object.  Device memory per channel: 144
 * bytes of members (64 and the history as two 300-bit strings: was it < 0, was it > 0), subframes_per_run =
 * GNSSHIP_LNAV_SUBFRAMES_PER_RUN(max_rounds) slots of 80 bytes, and 5 bytes per entry of a run (max_rounds of them). */
int gnsship_lnav_create(gnsship_ctx* ctx, const gnsship_lnav_conf* conf, int32_t max_channels, gnsship_lnav** out);
/* symbols[r*max_channels + c], r < n_rounds (0..max_rounds), float on the host or (on_device) on the device; valid and
 * flags180: uint8 of the same shape and place, or NULL for all valid / all false.  flags180 is read only where the block
 * seeds.  Channel c consumes its valid entries in order of r.  Outputs, in the handle's own device buffers
 * (gnsship_lnav_outputs_device) and copied to whichever host pointers are given:
 *   subframes[c][k], k < counts[c]   one record per successful decode and per failed state-1 decode, in order (failed
 *                                    state-0 attempts, one for about every 126 symbols of noise, are only counted in
 *                                    subframes_tried); slots beyond counts[c] are unspecified
 *   counts int32[c], faults uint8[c] faults: 1 where check_tlm_separation fired in this run
 *   tow_ms uint32[r*max_channels+c], sflags uint8[...]  r < n_rounds: the block's output stream — d_TOW_at_current_symbol_ms
 *                                    after the symbol and GNSSHIP_LNAV_S_*; both 0 for entries that are not symbols
 * With no host pointer the call is asynchronous on the context stream (host inputs then stay the caller's until the
 * stream has passed the run). */
int gnsship_lnav_run_symbols(gnsship_lnav* t, const float* symbols, const uint8_t* valid, const uint8_t* flags180, int on_device,
    int32_t n_rounds, gnsship_lnav_subframe* subframes_host, int32_t* counts_host, uint8_t* faults_host, uint32_t* tow_ms_host,
    uint8_t* sflags_host);
/* The same over tracking records of that shape: an entry is a symbol when flags & 1, the symbol is (float)prompt_i, the
 * 180° input is flags & 4, the subframe's sample_counter the completing record's. */
int gnsship_lnav_run_records(gnsship_lnav* t, const gnsship_trk_epoch* records, int on_device, int32_t n_rounds,
    gnsship_lnav_subframe* subframes_host, int32_t* counts_host, uint8_t* faults_host, uint32_t* tow_ms_host, uint8_t* sflags_host);
/* The same over the records the tracker's last run left on the device (gnsship_trk_records_device), in place, ordered
 * on the context stream; before or after gnsship_trk_collect.  n_rounds_out (may be NULL): the rounds of that run, the
 * first dimension of tow_ms / sflags.  E_STATE if there are no records; E_INVAL if the handles are on different
 * contexts, their max_channels differ or the run had more rounds than max_rounds. */
int gnsship_lnav_run_trk(gnsship_lnav* t, gnsship_trk* trk, gnsship_lnav_subframe* subframes_host, int32_t* counts_host,
    uint8_t* faults_host, uint32_t* tow_ms_host, uint8_t* sflags_host, int32_t* n_rounds_out);
/* The handle's output buffers (any pointer may be NULL) and subframes_per_run. */
int gnsship_lnav_outputs_device(gnsship_lnav* t, gnsship_lnav_subframe** subframes, int32_t** counts, uint8_t** faults,
    uint32_t** tow_ms, uint8_t** sflags, int32_t* subframes_per_run);
/* The block's reset() (:436-445): d_last_valid_preamble = d_sample_counter, the fault flag cleared, flag_TOW_set false,
 * the history cleared (the next symbol seeds again), d_stat 0.  The error counter, d_flag_frame_sync, the 180° flag, the
 * previous word, both TOW members and the navigation TOW stay. */
int gnsship_lnav_reset_channel(gnsship_lnav* t, int32_t channel);
/* set_satellite() (:217-224): a new navigation object — its TOW becomes 0, nothing else changes. */
int gnsship_lnav_set_satellite(gnsship_lnav* t, int32_t channel);
/* A new block object on this channel. */
int gnsship_lnav_new_channel(gnsship_lnav* t, int32_t channel);
/* The channel's members after everything run so far (waits for the context stream). */
int gnsship_lnav_state_get(gnsship_lnav* t, int32_t channel, gnsship_lnav_state* st);
int gnsship_lnav_destroy(gnsship_lnav* t);

/* ---------------------------------------------------------------------------------------------
 * GPS CNAV telemetry (L2C and L5) on the device: gps_l2c_telemetry_decoder_gs / gps_l5_telemetry_decoder_gs over
 * libswiftcnav (telemetry_decoder/libs/libswiftcnav: cnav_msg.c, viterbi27.c, bits.c, edc.c) up to the time of week, one
 * block object per channel, one wavefront per channel, integer arithmetic only (but for the L2C block's TOW, a double).
 * The library, restated and not repaired — all of this is part of the contract:
 *   parts       two K=7 rate-1/2 Viterbi decoders one symbol apart (cnav_msg.c:374-390: cnav_msg_decoder_init feeds
 *               part 2 one symbol of 0x80).  Each part buffers symbols, waits for 128 of them before its first decode and
 *               for 64 afterwards (:162-184), updates its decoder over all of them, chains back 64 bits and appends the
 *               oldest 32 to its 512-bit decode buffer (:194-199).
 *   update      viterbi27.c:85-189.  The symbol metric is (c0 ^ sym0) + (c1 ^ sym1) over the tables v27_poly_init makes of
 *               0x4F / 0x6D; the two candidates of a state are formed in uint32 arithmetic, modulo 2^32, the decision is
 *               (int32)(m0 - m1) > 0; bit j of the step's decision words w[0..1] is state j's.  Normalisation runs only
 *               when new_metrics[0] > 2^30 — state 0 alone is tested — and subtracts min(2^31, minimum over the states).
 *               The buffers are swapped at the end of every step.
 *   chain-back  v27_chainback_likely (:232-249) reads new_metrics, which after the swap holds the metrics of the step
 *               BEFORE the last; the start state is the first minimum of that stale buffer (ties: the lowest state), the
 *               walk still starts at the current decision index.  Both metric buffers are state.
 *   rescan      cnav_rescan_preamble_ (:117-145) looks for 0x8B / 0x74 from bit 1 (never bit 0) to n_decoded - 9; a hit
 *               sets `invert` and shifts the buffer to it; a miss leaves 7 bits.
 *   check       with a preamble and >= 300 bits, CRC-24Q over 276 bits against the last 24 (:227-275).  Without lock: a
 *               match locks, a mismatch drops the preamble and rescans the same buffer (the retry loop).  With lock: a
 *               mismatch counts, more than 10 in a row drop lock and preamble and rescan.
 *   dispose     cnav_msg_decode_ (:323-361) runs on every symbol while a part is locked and disposes of 300 bits whether
 *               the CRC held or not; crc_ok is whatever the last check left.  It returns true, with PRN, ID, TOW, alert,
 *               the un-inverted 64-byte buffer and delay = (n_decoded - 300 + 32) * 2 + n_symbols, only when crc_ok.
 *   precedence  (:415-439) part 1 locked: part 2's n_decoded and n_symbols are zeroed on every symbol (its buffers are
 *               not) and part 1 decodes; else the same with the parts exchanged.
 * The blocks, per symbol (L2C: gps_l2c_telemetry_decoder_gs.cc:189-344, L5: gps_l5_telemetry_decoder_gs.cc:191-360):
 *   symbol      (Prompt_I > 0) * 255 for L2C, (Prompt_Q > 0) * 255 for L5: a NaN or a zero of either sign is 0.
 *   watchdog    counter++, and once until reset() a fault when counter - last_valid_preamble > 3000 (L2C) / 6000 (L5).
 *               (L2C runs it after the decoder, L5 before; both before a message moves last_valid_preamble.)
 *   message     the 180° flag becomes part1.invert || part2.invert — including the stale `invert` of the part that is not
 *               locked.  L2C: last_valid_preamble = counter, the TOW, a double, becomes tow * 6.0 + delay * 0.02 +
 *               12 * 0.02 in that order, unfused, valid_word true.  L5: the TOW, integer ms, becomes tow * 6000 +
 *               (delay + 12) * 10; if the previous value is non-zero and differs by more than 10 ms, TOW and valid_word
 *               become 0; otherwise last_valid_preamble = counter and valid_word true.
 *   otherwise   L2C: TOW += 0.02, one addition per symbol (never k * 0.02), and valid_word drops on an entry whose
 *               output-valid flag is false.  L5: only while valid_word: TOW += 10, then the same drop.
 *   output      L2C: round(TOW * 1000) as uint32, valid_word and the 180° flag on every symbol.  L5: TOW and the 180° flag
 *               only while valid_word, else 0.
 *   reset()     L2C (:181-186): last_valid_preamble = counter, the fault flag cleared.  L5 (:181-188): also TOW and
 *               valid_word 0.  Neither touches the CNAV decoder.
 * Not here: Gps_CNAV_Navigation_Message::decode_page and the ephemeris, iono and UTC messages, the nav-data monitor, dumps,
 * the CRC-statistics option (which clears message_lock; it counts as off), and the pi added to the carrier phase (the
 * 180° flag is in the output instead). */
#define GNSSHIP_CNAV_MAX_CHANNELS (1 << 20)
#define GNSSHIP_CNAV_MAX_ROUNDS (1 << 20)
#define GNSSHIP_CNAV_L2C 0
#define GNSSHIP_CNAV_L5 1
/* The most records one run of max_rounds symbols can emit.  Every record disposes of 300 bits of a part's decode buffer.
 * A part gains 32 bits per decode; its decodes are 64 symbols apart, the first of a run at its first symbol at the
 * earliest (127 symbols held), so n symbols bring at most n / 64 + 2 decodes; and a part starts a run with at most 480
 * bits (331 in operation; 480 is what gnsship_cnav_state_set admits).  Both parts: 2 * (480 + 32 * (n / 64 + 2)) =
 * n + 1088 bits at most, hence R <= n / 300 + 4. */
#define GNSSHIP_CNAV_MESSAGES_PER_RUN(max_rounds) ((max_rounds) / 300 + 4)
typedef struct gnsship_cnav gnsship_cnav;
typedef struct gnsship_cnav_conf {
    int32_t max_rounds;      /* most entries per channel in one run, >= 1 */
    int32_t signal;          /* GNSSHIP_CNAV_L2C or GNSSHIP_CNAV_L5 */
    int32_t reserved;        /* 0 */
} gnsship_cnav_conf;
typedef struct gnsship_cnav_message { /* one 300-bit buffer a locked part disposed of, CRC good or not, 72 bytes */
    uint64_t symbol_counter;        /* d_sample_counter at the completing symbol */
    uint64_t sample_counter;        /* the completing epoch's record.sample_counter; 0 for run_symbols */
    int32_t channel;
    uint32_t tow;                   /* 17 bits, in 6-second units */
    uint32_t delay;                 /* (n_decoded - 300 + 32) * 2 + n_symbols */
    uint8_t prn, msg_id, alert;     /* bits 8..13, 14..19 and 37 of the un-inverted message */
    uint8_t part;                   /* 0: part 1, 1: part 2 */
    uint8_t raw[38];                /* the first 38 bytes of the un-inverted decode buffer: the 300 bits, MSB first */
    uint8_t flags;                  /* 1 crc_ok (the library returned true), 2 inverted, 4 message_lock after it */
    uint8_t reserved;
} gnsship_cnav_message;
typedef struct gnsship_cnav_part { /* cnav_v27_part_t with its v27_t, 1240 bytes */
    uint32_t metrics[2][64];        /* metrics1, metrics2 */
    uint32_t decisions[64][2];      /* v27_decision_t w[0..1] */
    uint8_t symbols[128];
    uint8_t decoded[64];
    uint32_t n_symbols, n_decoded, n_crc_fail, decisions_index;
    uint8_t old_is_metrics2;        /* old_metrics points at metrics2 (new_metrics at the other) */
    uint8_t preamble_seen, invert, message_lock, crc_ok, init;
    uint8_t reserved[2];
} gnsship_cnav_part;
typedef struct gnsship_cnav_state { /* every member of one block object, 2520 bytes */
    gnsship_cnav_part part[2];
    uint64_t symbol_counter, last_valid_preamble;
    double tow_s;                   /* L2C: d_TOW_at_current_symbol */
    uint32_t tow_ms;                /* L5: d_TOW_at_current_symbol_ms */
    uint32_t tow_at_preamble;       /* L2C: msg.tow; L5: msg.tow * 6000 */
    uint8_t pll_180, valid_word, sent_tlm_failed, reserved;
    uint32_t reserved2;
} gnsship_cnav_state;
#ifdef __cplusplus
static_assert(sizeof(gnsship_cnav_message) == 72, "gnsship_cnav_message");
static_assert(sizeof(gnsship_cnav_part) == 1240, "gnsship_cnav_part");
static_assert(sizeof(gnsship_cnav_state) == 2520, "gnsship_cnav_state");
#else
_Static_assert(sizeof(gnsship_cnav_message) == 72, "gnsship_cnav_message");
_Static_assert(sizeof(gnsship_cnav_part) == 1240, "gnsship_cnav_part");
_Static_assert(sizeof(gnsship_cnav_state) == 2520, "gnsship_cnav_state");
#endif
/* sflags of an entry */
#define GNSSHIP_CNAV_S_VALID_WORD 1 /* d_flag_valid_word after this symbol */
#define GNSSHIP_CNAV_S_PLL_180 2    /* the 180° flag as output with this symbol */
#define GNSSHIP_CNAV_S_MESSAGE 4    /* cnav_msg_decoder_add_symbol returned true here */
/* Channels 0..max_channels-1 (1..GNSSHIP_CNAV_MAX_CHANNELS), each a new block object: cnav_msg_decoder_init and zeroed
 * members.  Device memory per channel: 2520 bytes of members, messages_per_run =
 * GNSSHIP_CNAV_MESSAGES_PER_RUN(max_rounds) slots of 72 bytes, and 5 bytes per entry of a run (max_rounds of them). */
int gnsship_cnav_create(gnsship_ctx* ctx, const gnsship_cnav_conf* conf, int32_t max_channels, gnsship_cnav** out);
/* symbols[r*max_channels + c], r < n_rounds (0..max_rounds), float on the host or (on_device) on the device; valid and
 * out_valid: uint8 of the same shape and place, or NULL for all valid / all true (out_valid is the entry's
 * Flag_valid_symbol_output).  Channel c consumes its valid entries in order of r.  Outputs, in the handle's own device
 * buffers (gnsship_cnav_outputs_device) and copied to whichever host pointers are given:
 *   messages[c][k], k < counts[c]    one record per disposal, in order; slots beyond counts[c] are unspecified
 *   counts int32[c], faults uint8[c] faults: 1 where the watchdog fired in this run
 *   tow_ms uint32[r*max_channels+c], sflags uint8[...]  r < n_rounds: the block's output stream — the TOW in ms after the
 *                                    symbol and GNSSHIP_CNAV_S_*; both 0 for entries that are not symbols
 * With no host pointer the call is asynchronous on the context stream (host inputs then stay the caller's until the
 * stream has passed the run). */
int gnsship_cnav_run_symbols(gnsship_cnav* t, const float* symbols, const uint8_t* valid, const uint8_t* out_valid, int on_device,
    int32_t n_rounds, gnsship_cnav_message* messages_host, int32_t* counts_host, uint8_t* faults_host, uint32_t* tow_ms_host,
    uint8_t* sflags_host);
/* The same over tracking records of that shape: an entry is a symbol when flags & 1 and its output-valid flag is then
 * true; the symbol is prompt_i > 0 (L2C) or prompt_q > 0 (L5), asked of the double itself, not narrowed to float; the
 * message's sample_counter is the completing record's. */
int gnsship_cnav_run_records(gnsship_cnav* t, const gnsship_trk_epoch* records, int on_device, int32_t n_rounds,
    gnsship_cnav_message* messages_host, int32_t* counts_host, uint8_t* faults_host, uint32_t* tow_ms_host, uint8_t* sflags_host);
/* The same over the records the tracker's last run left on the device (gnsship_trk_records_device), in place, ordered
 * on the context stream; before or after gnsship_trk_collect.  n_rounds_out (may be NULL): the rounds of that run, the
 * first dimension of tow_ms / sflags.  E_STATE if there are no records; E_INVAL if the handles are on different
 * contexts, their max_channels differ or the run had more rounds than max_rounds. */
int gnsship_cnav_run_trk(gnsship_cnav* t, gnsship_trk* trk, gnsship_cnav_message* messages_host, int32_t* counts_host,
    uint8_t* faults_host, uint32_t* tow_ms_host, uint8_t* sflags_host, int32_t* n_rounds_out);
/* The handle's output buffers (any pointer may be NULL) and messages_per_run. */
int gnsship_cnav_outputs_device(gnsship_cnav* t, gnsship_cnav_message** messages, int32_t** counts, uint8_t** faults,
    uint32_t** tow_ms, uint8_t** sflags, int32_t* messages_per_run);
/* The block's reset(): last_valid_preamble = counter, the fault flag cleared; L5 also TOW and valid_word 0. */
int gnsship_cnav_reset_channel(gnsship_cnav* t, int32_t channel);
/* A new block object on this channel. */
int gnsship_cnav_new_channel(gnsship_cnav* t, int32_t channel);
/* The channel's members after everything run so far (waits for the context stream). */
int gnsship_cnav_state_get(gnsship_cnav* t, int32_t channel, gnsship_cnav_state* st);
/* The channel's members become *st (ordered on the context stream; *st is copied before the call returns): a channel
 * moves between handles, or starts from a state the stream would take hours to reach.  E_INVAL unless, per part,
 * n_symbols < 128 (init) or 64, n_decoded <= 480, decisions_index < 64 and the flags are 0 or 1. */
int gnsship_cnav_state_set(gnsship_cnav* t, int32_t channel, const gnsship_cnav_state* st);
int gnsship_cnav_destroy(gnsship_cnav* t);

/* ---------------------------------------------------------------------------------------------
 * BeiDou D1/D2 telemetry (B1I and B3I) on the device: beidou_b1i_telemetry_decoder_gs / beidou_b3i_telemetry_decoder_gs
 * with what they use of Beidou_Dnav_Navigation_Message (d1_subframe_decoder, d2_subframe_decoder) up to the time of week,
 * one block object per channel, one wavefront per channel, no float arithmetic beyond the sign tests.  The two blocks are
 * one algorithm with a signal mode.  Restated and not repaired — all of this is part of the contract:
 *   history      a circular buffer of 311 (300 + 11) floats; every symbol is pushed as (float)Prompt_I and d_sample_counter
 *                grows by one.  reset() and set_satellite() keep its contents.
 *   correlation  only when the history holds 311 entries: over the 11 oldest against "11100010010", -preamble where the
 *                entry is < 0 and +preamble otherwise, so +0, -0 and NaN count as positive.  A hit is |corr| >= 11.
 *   state 0      a hit sets preamble_index = counter and state 1.
 *   state 1      on a hit only, with diff = (int32)(counter - preamble_index): diff == 300 decodes and the outcome is
 *                state 2; diff > 300 goes back to state 0 and this hit is thrown away; diff < 300 does nothing.  Without a
 *                hit state 1 never times out.
 *   state 2      when counter == preamble_index + 300: decode, hit or not.
 *   polarity     in both decodes normal when corr > 0, inverted otherwise: a state-2 subframe whose preamble did not match
 *                (corr 0, -3, ...) is decoded inverted.  The 300 symbols decoded are the 300 oldest history entries.
 *   decode       a bit is +1 when the (possibly negated) float is > 0, else -1: zero and NaN are -1 under both polarities.
 *                Word 1 is taken as it is.  Words 2..10 are de-interleaved (enc[c*2 + r] to row r, column c), each row goes
 *                through decode_bch15_11_01 (a syndrome of 1..15 flips one bit, whatever the true error was), and the word
 *                is 11 + 11 information bits, then 4 + 4 parity bits.
 *   D1 / D2      the blocks differ.  B1I uses the D2 decoder and the D2 timing (2 ms per symbol) for PRN 1..5 or > 58.  B3I
 *                uses the D2 decoder for PRN 1..5 only, but the D2 timing for PRN 1..5 or > 58: a B3I PRN > 58 runs the
 *                D1 decoder with 2 ms symbols.  Otherwise D1 and 20 ms.
 *   nav object   flag_crc_test is always true (the CRC is "tbd" in the source), so d_CRC_error_counter stays 0, frame sync
 *                is never lost and an object in state 2 stays there; the branch behind `> CRC_ERROR_LIMIT` is unreachable
 *                and is not here.  D1: FraID is bits 16..18, read whatever the preamble; for FraID 1..5 d_SOW becomes bits
 *                19..26 ‖ 31..42 and flag_new_SOW_available is set, any other FraID leaves both alone.  D2: only FraID 1
 *                with Pnum (bits 43..46) in 1..10 does so.  The block clears the flag when it uses it.
 *   stamp        on a decode with the flag set: tow_at_preamble_ms = (SOW + 14) * 1000, tow_at_current_symbol_ms = that +
 *                311 * symbol_duration_ms; if the previous current-symbol value was non-zero and differs from the new one
 *                by more than one symbol duration (int64 arithmetic) the result is TOW 0 and valid_word false, otherwise
 *                last_valid_preamble = counter and valid_word true.  On every other symbol, while valid_word: the TOW
 *                grows by one symbol duration, and valid_word falls if the entry's output-valid flag is false.  The block
 *                outputs the symbol only while valid_word.
 *   reset()      last_valid_preamble = counter, TOW 0, valid_word false, the fault flag cleared; nothing else: state,
 *                preamble_index and history stay.
 *   faults       the blocks never publish on telemetry_to_trk: there is no fault output.
 * Not here: ephemeris, almanac, iono and UTC fields and their messages, the nav-data monitor, CRC statistics, dumps. */
#define GNSSHIP_DNAV_MAX_CHANNELS (1 << 20)
#define GNSSHIP_DNAV_MAX_ROUNDS (1 << 20)
#define GNSSHIP_DNAV_B1I 0
#define GNSSHIP_DNAV_B3I 1
/* The most records one run of max_rounds symbols can emit.  A record is a decode.  Every decode sets preamble_index =
 * counter and leaves state 2, which is never left; in state 2 the only decode is the one at counter == preamble_index +
 * 300.  So a run's decodes after its first are exactly 300 symbols apart, and the first (a state-1 hit, or the due symbol
 * of state 2) falls on the run's first symbol at the earliest: n symbols hold at most (n - 1) / 300 + 1 <= n / 300 + 1
 * decodes, and n = 300 k + 1 symbols starting on a due symbol hold exactly k + 1. */
#define GNSSHIP_DNAV_SUBFRAMES_PER_RUN(max_rounds) ((max_rounds) / 300 + 1)
typedef struct gnsship_dnav gnsship_dnav;
typedef struct gnsship_dnav_conf {
    int32_t max_rounds;      /* most entries per channel in one run, >= 1 */
    int32_t signal;          /* GNSSHIP_DNAV_B1I or GNSSHIP_DNAV_B3I */
    int32_t reserved;        /* 0 */
} gnsship_dnav_conf;
/* gnsship_dnav_subframe.flags */
#define GNSSHIP_DNAV_INVERTED 1    /* decoded under the inverted polarity (corr <= 0) */
#define GNSSHIP_DNAV_STATE1 2      /* decoded in state 1 (a hit 300 symbols after a hit); otherwise in state 2 */
#define GNSSHIP_DNAV_NEW_SOW 4     /* flag_new_SOW_available was set: the stamp ran here */
#define GNSSHIP_DNAV_D2_DECODER 8  /* d2_subframe_decoder; otherwise d1_subframe_decoder */
#define GNSSHIP_DNAV_D2_TIMING 16  /* 2 ms per symbol; otherwise 20 ms */
#define GNSSHIP_DNAV_TOW_ZEROED 32 /* the TOW consistency check failed here: TOW 0, valid_word false */
typedef struct gnsship_dnav_subframe { /* one decode, 88 bytes */
    uint64_t symbol_counter;        /* d_sample_counter at the completing symbol */
    uint64_t sample_counter;        /* the completing epoch's record.sample_counter; 0 for run_symbols */
    uint32_t words[10];             /* the ten decoded 30-bit words, bit 1 of the word in bit 29 */
    int32_t channel;
    int32_t fra_id;                 /* bits 16..18 */
    int32_t pnum;                   /* bits 43..46 under the D2 decoder, bits 44..50 under D1, whatever the ID */
    uint32_t sow;                   /* the navigation object's d_SOW after the decode */
    uint32_t corrected_mask;        /* bit 2(w-2)+r: the syndrome of row r of word w (2..10) was non-zero */
    uint32_t tow_at_current_symbol_ms; /* after the stamp */
    uint32_t flags;                 /* GNSSHIP_DNAV_* above */
    uint32_t reserved;
} gnsship_dnav_subframe;
typedef struct gnsship_dnav_state { /* every member of one block object that the above names, 64 bytes */
    uint64_t symbol_counter;        /* d_sample_counter */
    uint64_t preamble_index;
    uint64_t last_valid_preamble;
    uint32_t tow_at_preamble_ms, tow_at_current_symbol_ms;
    uint32_t sow;                   /* the navigation object's d_SOW (a double there; always an integer below 2^20) */
    uint32_t symbol_duration_ms;    /* 20 or 2 */
    int32_t stat;
    int32_t crc_error_counter;      /* always 0 */
    int32_t history_size;           /* 0..311 */
    int32_t prn;
    uint8_t sow_set, frame_sync, valid_word;
    uint8_t new_sow_available;      /* the navigation object's flag between symbols: always 0, the block uses it at once */
    uint8_t sent_tlm_failed;        /* never set; reset() clears it */
    uint8_t d2_decoder, d2_timing;  /* what set_satellite chose for the PRN */
    uint8_t reserved;
} gnsship_dnav_state;
#ifdef __cplusplus
static_assert(sizeof(gnsship_dnav_subframe) == 88, "gnsship_dnav_subframe");
static_assert(sizeof(gnsship_dnav_state) == 64, "gnsship_dnav_state");
#else
_Static_assert(sizeof(gnsship_dnav_subframe) == 88, "gnsship_dnav_subframe");
_Static_assert(sizeof(gnsship_dnav_state) == 64, "gnsship_dnav_state");
#endif
/* sflags of an entry */
#define GNSSHIP_DNAV_S_VALID_WORD 1 /* d_flag_valid_word after this symbol: the block outputs it */
#define GNSSHIP_DNAV_S_SUBFRAME 2   /* a subframe was decoded at this symbol */
#define GNSSHIP_DNAV_S_INVERTED 4   /* ... under the inverted polarity */
/* Channels 0..max_channels-1 (1..GNSSHIP_DNAV_MAX_CHANNELS), each a new block object on PRN 0 (D1, 20 ms).  Device memory
 * per channel: 144 bytes of members and history (two 311-bit strings: "was < 0", "was > 0"), subframes_per_run =
 * GNSSHIP_DNAV_SUBFRAMES_PER_RUN(max_rounds) slots of 88 bytes, and 5 bytes per entry of a run (max_rounds of them). */
int gnsship_dnav_create(gnsship_ctx* ctx, const gnsship_dnav_conf* conf, int32_t max_channels, gnsship_dnav** out);
/* symbols[r*max_channels + c], r < n_rounds (0..max_rounds), float on the host or (on_device) on the device; valid and
 * out_valid: uint8 of the same shape and place, or NULL for all valid / all true (out_valid is the entry's
 * Flag_valid_symbol_output).  Channel c consumes its valid entries in order of r.  Outputs, in the handle's own device
 * buffers (gnsship_dnav_outputs_device) and copied to whichever host pointers are given:
 *   subframes[c][k], k < counts[c]   one record per decode, in order; slots beyond counts[c] are unspecified
 *   counts int32[c]
 *   tow_ms uint32[r*max_channels+c], sflags uint8[...]  r < n_rounds: d_TOW_at_current_symbol_ms after the symbol (the
 *                                    block outputs it only with GNSSHIP_DNAV_S_VALID_WORD) and GNSSHIP_DNAV_S_*; both 0
 *                                    for entries that are not symbols
 * With no host pointer the call is asynchronous on the context stream (host inputs then stay the caller's until the
 * stream has passed the run). */
int gnsship_dnav_run_symbols(gnsship_dnav* t, const float* symbols, const uint8_t* valid, const uint8_t* out_valid, int on_device,
    int32_t n_rounds, gnsship_dnav_subframe* subframes_host, int32_t* counts_host, uint32_t* tow_ms_host, uint8_t* sflags_host);
/* The same over tracking records of that shape: an entry is a symbol when flags & 1, the symbol is (float)prompt_i and
 * its output-valid flag is then true; the subframe's sample_counter is the completing record's. */
int gnsship_dnav_run_records(gnsship_dnav* t, const gnsship_trk_epoch* records, int on_device, int32_t n_rounds,
    gnsship_dnav_subframe* subframes_host, int32_t* counts_host, uint32_t* tow_ms_host, uint8_t* sflags_host);
/* The same over the records the tracker's last run left on the device (gnsship_trk_records_device), in place, ordered
 * on the context stream; before or after gnsship_trk_collect.  n_rounds_out (may be NULL): the rounds of that run, the
 * first dimension of tow_ms / sflags.  E_STATE if there are no records; E_INVAL if the handles are on different
 * contexts, their max_channels differ or the run had more rounds than max_rounds. */
int gnsship_dnav_run_trk(gnsship_dnav* t, gnsship_trk* trk, gnsship_dnav_subframe* subframes_host, int32_t* counts_host,
    uint32_t* tow_ms_host, uint8_t* sflags_host, int32_t* n_rounds_out);
/* The handle's output buffers (any pointer may be NULL) and subframes_per_run. */
int gnsship_dnav_outputs_device(gnsship_dnav* t, gnsship_dnav_subframe** subframes, int32_t** counts, uint32_t** tow_ms,
    uint8_t** sflags, int32_t* subframes_per_run);
/* The block's reset(). */
int gnsship_dnav_reset_channel(gnsship_dnav* t, int32_t channel);
/* The block's set_satellite(): the PRN (0..63), the symbol duration and the decoder choice; nothing else moves. */
int gnsship_dnav_set_satellite(gnsship_dnav* t, int32_t channel, int32_t prn);
/* A new block object on this channel, constructed on this PRN. */
int gnsship_dnav_new_channel(gnsship_dnav* t, int32_t channel, int32_t prn);
/* The channel's members after everything run so far (waits for the context stream). */
int gnsship_dnav_state_get(gnsship_dnav* t, int32_t channel, gnsship_dnav_state* st);
int gnsship_dnav_destroy(gnsship_dnav* t);

/* ---------------------------------------------------------------------------------------------
 * GLONASS GNAV telemetry (L1 C/A and L2 C/A) on the device: glonass_l1_ca_telemetry_decoder_gs / glonass_l2_ca_telemetry_decoder_gs
 * with what they use of Glonass_Gnav_Navigation_Message (CRC_test, string_decoder, have_new_ephemeris, have_new_utc_model)
 * and Glonass_Gnav_Ephemeris::glot_to_gpst up to the time of week.  One block object per channel, one lane per channel.
 * The two blocks are one algorithm (they differ in names and log text; the L2 block repeats its valid-word test), so the
 * signal only names the handle.  Restated and not repaired — all of this is part of the contract:
 *   history      a ring of capacity 2000; every symbol is pushed (its double Prompt_I) and d_sample_counter grows by one.
 *   correlation  as soon as the history holds 300 entries, over its 300 OLDEST entries against the 30 time-mark bits
 *                "111110001101110101000010010110" at 10 symbols each: -preamble where the entry is < 0.0, +preamble otherwise
 *                (NaN, +0 and -0 count as +1).  While the ring is filling (fewer than 2000 entries) these are the first 300
 *                symbols ever received, tested again on every symbol.  A hit is |corr| >= 300.
 *   state 0      a hit sets preamble_index = counter and state 1.
 *   state 1      on a hit only, with diff = (int32)(counter - preamble_index): diff == 2000 sets preamble_index = counter
 *                and state 2 (nothing is decoded); diff > 2000 goes back to state 0 and the hit is thrown away; diff < 2000
 *                does nothing.  Without a hit state 1 never times out.
 *   state 2      hits are ignored.  When counter == preamble_index + 2000 the string is decoded whatever corr is; its
 *                polarity is normal when corr > 0 and inverted when corr <= 0 (a time mark that did not match decodes
 *                inverted when corr is 0 or negative).  The symbols decoded are history entries 300..1999.
 *   decode       170 half-bits, each `sum > 0` of a double sum of 10 consecutive symbols added in order from 0.0; under
 *                the inverted polarity every symbol is negated first, which is exact, so the half-bit is `sum < 0`: a NaN or
 *                zero sum is '0' under both.  Half-bit pair "10" is relative bit 1, any other pair 0.  Data bit 0 is '0',
 *                data bit i is relative bit i-1 XOR relative bit i.  Character i of the 85 enters the bitset as bit 84 - i.
 *   CRC_test     eight parities C1..C7, C_Sigma (C_Sigma is the parity of all 85 bits).  In this order: (1) all eight zero:
 *                accept.  (2) C_Sigma == 1 and exactly one of C1..C7 set: accept, nothing flipped.  (3) C_Sigma == 1 and the
 *                parity of bits 8..84 odd: the syndrome C1 + 2 C2 + ... + 64 C7, when below 85, flips bits[locator[syndrome]]
 *                and accepts; 85 or above rejects.  (4) reject.  In (3) the syndromes 1, 2, 4, ..., 64 cannot occur (branch 2
 *                took them); syndrome 0 can, and flips bit 0.  A C_Sigma == 1 word with even parity over bits 8..84 is
 *                rejected even where its syndrome names one bit.
 *   nav object   a rejected string changes nothing.  String 1 sets t_k = 3600 h + 60 m + 30 s and flag 1.  Strings 2, 3, 4, 5
 *                are read only if the flag of the string before is set: string 2 sets t_b (15-minute units, in seconds),
 *                string 4 N_T, n and flag_update_slot_number, string 5 tau_c (sign-magnitude 32 bits, 2^-31), N_4, tau_gps
 *                (sign-magnitude 22 bits, 2^-30), flag_utc_model_str_5 and, if flag 1 is set, d_WN / d_TOW with flag_TOW_set
 *                and flag_TOW_new.  After every decode, accepted or not, have_new_ephemeris() and have_new_utc_model() run:
 *                the first clears flags 1..4 when all four and the UTC flag are set and t_b differs from d_previous_tb (which
 *                starts at 0, so a satellite with t_b == 0 never clears them); the second clears the UTC flag.  After string
 *                4 the channel's PRN becomes n.  Almanac strings (6..15) touch nothing here.
 *   glot_to_gpst integer dates: 1 January of 1996 + 4 (N_4 - 1), plus N_T - 1 days, plus t_k + 10 - 10800 seconds (which may
 *                be negative, or more than a day).  The leap seconds are those of the first table entry (2017: 18, 2015: 17,
 *                2012: 16, 2009: 15, 2006: 14, 1999: 13, 1 July 1997: 12, 1996: 11, 1 July 1994: 10, 1993: 9, 1992: 8,
 *                1991: 7, ...) at or before that instant.  days is counted from 6 January 1980 to the UTC date, the
 *                seconds of day are those of the GPS instant: a leap addition that crosses midnight is a day short.
 *                d_WN = floor(total / 604800), d_TOW = total - 604800 floor(total / 604800), then d_TOW += (tau_c + tau_gps).
 *   CRC counter  an accepted string zeroes it, raises d_flag_preamble for this symbol and sets frame sync; a rejected one
 *                counts up and above 6 drops frame sync and returns to state 0.  Both set preamble_index = counter.
 *   stamp        doubles throughout, IEEE divide, nothing contracted (the library is built with -ffp-contract=off): on an
 *                accepted decode with flag_TOW_new, d_TOW_at_current_symbol = floor((d_TOW - 0.3) * 1000) / 1000; on every
 *                other symbol it is + 0.001.  The output is round(x * 1000.0) (half away from zero) into a uint32: for a
 *                negative value the block's conversion is undefined, and device and model take the low 32 bits of the int64
 *                value, as an x86-64 build does.  Flag_valid_word is d_flag_frame_sync && flag_TOW_set.
 *   faults       the blocks never publish on telemetry_to_trk: there is no fault output.  Flag_valid_symbol_output is not read.
 * Not here: ephemeris, almanac and UTC fields and their messages (the record carries the 85 bits), the nav-data monitor,
 * CRC statistics, dumps, the GLONASS-to-GPS offset the block leaves commented out. */
#define GNSSHIP_GNAV_MAX_CHANNELS (1 << 20)
#define GNSSHIP_GNAV_MAX_ROUNDS (1 << 20)
#define GNSSHIP_GNAV_L1CA 0
#define GNSSHIP_GNAV_L2CA 1
/* The most records one run of max_rounds symbols can emit.  A record is a decode, and a decode happens only in state 2 at
 * counter == preamble_index + 2000.  Every decode sets preamble_index = counter, and so does the entry into state 2: the
 * next decode, whether state 2 was kept or left and entered again, is at least 2000 symbols later.  A run's first decode
 * falls on its first symbol at the earliest, so n symbols hold at most (n - 1) / 2000 + 1 <= n / 2000 + 1 decodes, and
 * n = 2000 k + 1 symbols starting on a due symbol of a channel that keeps state 2 hold exactly k + 1. */
#define GNSSHIP_GNAV_STRINGS_PER_RUN(max_rounds) ((max_rounds) / 2000 + 1)
typedef struct gnsship_gnav gnsship_gnav;
typedef struct gnsship_gnav_conf {
    int32_t max_rounds;      /* most entries per channel in one run, >= 1 */
    int32_t signal;          /* GNSSHIP_GNAV_L1CA or GNSSHIP_GNAV_L2CA */
    int32_t reserved;        /* 0 */
} gnsship_gnav_conf;
/* gnsship_gnav_string.flags */
#define GNSSHIP_GNAV_CRC_OK 1        /* CRC_test accepted the string */
#define GNSSHIP_GNAV_CORRECTED 2     /* ... after flipping bit flipped_bit */
#define GNSSHIP_GNAV_INVERTED 4      /* decoded under the inverted polarity (corr <= 0) */
#define GNSSHIP_GNAV_NEW_TOW 8       /* flag_TOW_new was set: the stamp was taken from d_TOW here */
#define GNSSHIP_GNAV_SLOT_UPDATED 16 /* flag_update_slot_number: the PRN became n */
#define GNSSHIP_GNAV_NEW_EPHEMERIS 32 /* have_new_ephemeris() returned true */
#define GNSSHIP_GNAV_NEW_UTC_MODEL 64 /* have_new_utc_model() returned true */
typedef struct gnsship_gnav_string { /* one decode, 64 bytes */
    uint64_t symbol_counter;        /* d_sample_counter at the completing symbol */
    uint64_t sample_counter;        /* the completing epoch's record.sample_counter; 0 for run_symbols */
    double tow;                     /* the navigation object's d_TOW after the decode */
    uint32_t bits[3];               /* the bitset after CRC_test: bit i in bits[i / 32] bit i % 32, i < 85 */
    int32_t channel;
    int32_t prn;                    /* the channel's PRN after the decode */
    int32_t string_id;              /* bits 83..80, whatever CRC_test said */
    int32_t flipped_bit;            /* the bit CRC_test flipped, or -1 */
    uint32_t tow_at_current_symbol_ms; /* the block's output at this symbol */
    uint32_t flags;                 /* GNSSHIP_GNAV_* above */
    uint32_t reserved;
} gnsship_gnav_string;
typedef struct gnsship_gnav_state { /* every member of one block object and its navigation object that the above names, 416 bytes */
    uint64_t symbol_counter;        /* d_sample_counter */
    uint64_t preamble_index;
    double tow_at_current_symbol;   /* d_TOW_at_current_symbol, seconds */
    double tow;                     /* d_TOW */
    double tau_c, tau_gps;
    double chip_acc;                /* the half-bit sum in flight (state 2, between two half-bit boundaries) */
    int32_t stat;
    int32_t crc_error_counter;
    int32_t history_size;           /* min(symbol_counter, 2000) */
    int32_t prn;
    int32_t wn;                     /* d_WN */
    uint32_t t_k, t_b, previous_tb; /* seconds; doubles in the source, always integers */
    uint32_t n_t, n, n_4;
    uint8_t frame_sync;
    uint8_t ephemeris_str[4];       /* flag_ephemeris_str_1..4 */
    uint8_t utc_model_str_5;        /* always 0 between symbols: have_new_utc_model() clears it after every decode */
    uint8_t tow_set, tow_new;       /* tow_new is always 0 between symbols: the block uses it at once */
    uint8_t reserved[4];
    /* Of state 2, where data symbol j (0..1699) is the one with counter preamble_index + 301 + j: half-bit h = j / 10 is
     * complete once its tenth symbol has come; bit h % 32 of half_pos[h / 32] is `sum > 0`, of half_neg `sum < 0`.
     * chip_acc is 0.0 after a complete half-bit.  Every decode clears all three, so outside state 2 they are zero. */
    uint32_t half_pos[6], half_neg[6];
    /* "Prompt_I < 0.0" of the last history_size symbols: the symbol pushed when the counter became k is bit (k % 2000) % 32
     * of history[(k % 2000) / 32]. */
    uint32_t history[64];
} gnsship_gnav_state;
#ifdef __cplusplus
static_assert(sizeof(gnsship_gnav_string) == 64, "gnsship_gnav_string");
static_assert(sizeof(gnsship_gnav_state) == 416, "gnsship_gnav_state");
#else
_Static_assert(sizeof(gnsship_gnav_string) == 64, "gnsship_gnav_string");
_Static_assert(sizeof(gnsship_gnav_state) == 416, "gnsship_gnav_state");
#endif
/* sflags of an entry */
#define GNSSHIP_GNAV_S_VALID_WORD 1 /* Flag_valid_word of this symbol */
#define GNSSHIP_GNAV_S_STRING 2     /* a string was decoded at this symbol */
#define GNSSHIP_GNAV_S_INVERTED 4   /* ... under the inverted polarity */
/* Channels 0..max_channels-1 (1..GNSSHIP_GNAV_MAX_CHANNELS), each a new block object on PRN 0.  Device memory per channel:
 * 416 bytes of members (the history is 2000 sign bits, the string in flight two 170-bit strings and one double),
 * strings_per_run = GNSSHIP_GNAV_STRINGS_PER_RUN(max_rounds) slots of 64 bytes, and 5 bytes per entry of a run. */
int gnsship_gnav_create(gnsship_ctx* ctx, const gnsship_gnav_conf* conf, int32_t max_channels, gnsship_gnav** out);
/* symbols[r*max_channels + c], r < n_rounds (0..max_rounds), float on the host or (on_device) on the device, widened to
 * double; valid and out_valid: uint8 of the same shape and place, or NULL.  Channel c consumes its valid entries in order
 * of r.  out_valid is the entry's Flag_valid_symbol_output, which these blocks never read: it is accepted for the shape of
 * the call and changes nothing.  Outputs, in the handle's own device buffers (gnsship_gnav_outputs_device) and copied to
 * whichever host pointers are given:
 *   strings[c][k], k < counts[c]     one record per decode, in order; slots beyond counts[c] are unspecified
 *   counts int32[c]
 *   tow_ms uint32[r*max_channels+c], sflags uint8[...]  r < n_rounds: TOW_at_current_symbol_ms of the symbol and
 *                                    GNSSHIP_GNAV_S_*; both 0 for entries that are not symbols
 * With no host pointer the call is asynchronous on the context stream (host inputs then stay the caller's until the
 * stream has passed the run).  Any cut of a stream into runs gives the same outputs. */
int gnsship_gnav_run_symbols(gnsship_gnav* t, const float* symbols, const uint8_t* valid, const uint8_t* out_valid, int on_device,
    int32_t n_rounds, gnsship_gnav_string* strings_host, int32_t* counts_host, uint32_t* tow_ms_host, uint8_t* sflags_host);
/* The same over tracking records of that shape: an entry is a symbol when flags & 1, the symbol is the record's double
 * prompt_i; the string's sample_counter is the completing record's. */
int gnsship_gnav_run_records(gnsship_gnav* t, const gnsship_trk_epoch* records, int on_device, int32_t n_rounds,
    gnsship_gnav_string* strings_host, int32_t* counts_host, uint32_t* tow_ms_host, uint8_t* sflags_host);
/* The same over the records the tracker's last run left on the device (gnsship_trk_records_device), in place, ordered
 * on the context stream.  n_rounds_out (may be NULL): the rounds of that run.  E_STATE if there are no records; E_INVAL if
 * the handles are on different contexts, their max_channels differ or the run had more rounds than max_rounds. */
int gnsship_gnav_run_trk(gnsship_gnav* t, gnsship_trk* trk, gnsship_gnav_string* strings_host, int32_t* counts_host,
    uint32_t* tow_ms_host, uint8_t* sflags_host, int32_t* n_rounds_out);
/* The handle's output buffers (any pointer may be NULL) and strings_per_run. */
int gnsship_gnav_outputs_device(gnsship_gnav* t, gnsship_gnav_string** strings, int32_t** counts, uint32_t** tow_ms,
    uint8_t** sflags, int32_t* strings_per_run);
/* The block's set_satellite(): the PRN (0..63); nothing else moves. */
int gnsship_gnav_set_satellite(gnsship_gnav* t, int32_t channel, int32_t prn);
/* A new block object on this channel, constructed on this PRN. */
int gnsship_gnav_new_channel(gnsship_gnav* t, int32_t channel, int32_t prn);
/* The channel's members after everything run so far (waits for the context stream). */
int gnsship_gnav_state_get(gnsship_gnav* t, int32_t channel, gnsship_gnav_state* st);
/* The channel's members become *st (ordered on the context stream; *st is copied before the call returns): a channel
 * moves between handles, or starts from a state the stream would take many seconds to reach.  E_INVAL unless stat is
 * 0..2, history_size == min(symbol_counter, 2000), crc_error_counter >= 0 and the flags are 0 or 1. */
int gnsship_gnav_state_set(gnsship_gnav* t, int32_t channel, const gnsship_gnav_state* st);
int gnsship_gnav_destroy(gnsship_gnav* t);

/* ------------------------------------------------------------------------------------------ */
/* Multi-GPU fan-out: one process per GPU, one RCCL communicator per context.  */
/* The reference connects one conditioner output to every channel block (gnss_flowgraph.cc:    */
/* 1127-1136); across GPUs that connection is a broadcast of the raw IF block from the rank     */
/* that reads the front end, after which every rank tracks / acquires its own channel or PRN    */
/* shard with no further data-path collective.  Collectives are enqueued on the context stream  */
/* (ordered before any later launch of that context; gnsship_ctx_sync waits for them).          */
/* ------------------------------------------------------------------------------------------ */
typedef struct gnsship_comm gnsship_comm;
#define GNSSHIP_COMM_ID_BYTES 128
/* Rank 0 creates the id and hands it to the other ranks out of band (e.g. the launcher's store). */
int gnsship_comm_unique_id(void* id);
int gnsship_comm_create(gnsship_ctx* ctx, int n_ranks, int rank, const void* id, gnsship_comm** out);
int gnsship_comm_rank(gnsship_comm* c, int* rank, int* n_ranks);
/* In-place broadcast of `bytes` of a device buffer from `root` (raw IF samples in any format). */
int gnsship_comm_broadcast(gnsship_comm* c, void* dev_buf, size_t bytes, int root);
/* dev_recv[r·bytes_per_rank ...] = rank r's dev_send (per-PRN acquisition results, records). */
int gnsship_comm_allgather(gnsship_comm* c, const void* dev_send, void* dev_recv, size_t bytes_per_rank);
/* In-place max over ranks of `count` doubles (timing: the slowest rank's wall time). */
int gnsship_comm_allreduce_max_f64(gnsship_comm* c, double* dev_buf, size_t count);
int gnsship_comm_destroy(gnsship_comm* c);

#ifdef __cplusplus
}
#endif
#endif /* GNSSHIP_H */
