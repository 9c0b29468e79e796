// trk_glo_loop.h — the per-epoch loop of glonass_l1_ca_dll_pll_tracking_cc (and its L2 twin, the same text with the
// L2 constants) as one device function, run by thread 0 of trk_persist.hip's generic serial pipeline in place of the
// epoch_pre / lock_status / epoch_loop / epoch_post / epoch_finish phases of dll_pll_veml_tracking (trk_loop.h).
//
// general_work :526-629 in its own order and types:
//   taps (E, P, L) → pll_cloop_two_quadrant_atan / 2π → Tracking_2nd_PLL_filter (float) → both frequencies, then
//   d_code_freq_chips from d_glonass_freq_ch → dll_nc_e_minus_l_normalized(E, L, spc, 1.0) → Tracking_2nd_DLL_filter
//   (float) → K_blk_samples and the new block length → NCO commands (d_rem_carr_phase_rad a float: a float-cast
//   product added, then fmod against the double 2π) → remnant code phase → the lock test: CN0_ESTIMATION_SAMPLES
//   prompts stored, the next epoch (its prompt not stored) tests them over the full length.
// The epoch is correlated over the block length the PREVIOUS epoch left (:529-533) and consumes the NEW one (:705-707).
//
// The block's members live in TrkChannel.  Those dll_pll_veml_tracking has no counterpart for reuse members this block
// never touches otherwise:
//   d_carrier_frequency_hz (Doppler + FDMA offset)   carrier_phase_rate_step_rad
//   (double)d_glonass_freq_ch                        code_phase_rate_step_chips
//   PLL filter d_old_carr_nco / d_old_carr_error     fp_w / fp_x
//   DLL filter d_old_code_nco / d_old_code_error     lf_outputs[0] / lf_inputs[0]
//   d_carrier_phase_step_rad (with the offset)       carrier_phase_step_rad
//   d_cn0_estimation_counter, d_Prompt_buffer        cn0_counter, prompt_buf
//   d_carrier_lock_fail_counter                      carrier_fail
// and the filters' two constants each, fixed at create time (ζ = 0.7, k = 1 / 0.25, pdi = 1 ms), in TrkParams::ls[0]:
//   lf_in[0] = tau2_code / tau1_code, lf_in[1] = pdi / (2·tau1_code); lf_out[0], lf_out[1] the carrier filter's.
#pragma once
#include "trk_loop.h"

namespace gnsship {
namespace {

constexpr int kGloCn0EstimationSamples = 10;  // CN0_ESTIMATION_SAMPLES (glonass_l1_ca_dll_pll_tracking_cc.cc:47)

// carrier_lock_detector over a general length (lock_detectors.cc:130-147): the two serial float sums, then
// (I² − Q²) / (I² + Q²).  trk_loop.h has the length-1 form dll_pll_veml_tracking calls.
__device__ __forceinline__ float carrier_lock_detector_n(const float* prompt, int length)
{
    float si = 0.0f, sq = 0.0f;
    for (int i = 0; i < length; i++) {
        si = __fadd_rn(si, prompt[2 * i]);
        sq = __fadd_rn(sq, prompt[2 * i + 1]);
    }
    const float nbp = __fadd_rn(__fmul_rn(si, si), __fmul_rn(sq, sq));
    const float nbd = __fsub_rn(__fmul_rn(si, si), __fmul_rn(sq, sq));
    return __fdiv_rn(nbd, nbp);
}

// Tracking_2nd_DLL_filter::get_code_nco / Tracking_2nd_PLL_filter::get_carrier_nco (tracking_2nd_DLL_filter.cc:52-58,
// tracking_2nd_PLL_filter.cc:57-63): old_nco + (tau2 / tau1)·(x − old_error) + (x + old_error)·(pdi / (2·tau1)), float.
__device__ __forceinline__ float glo_filter(float& old_nco, float& old_error, float ratio, float gain, float x)
{
    const float nco = __fadd_rn(__fadd_rn(old_nco, __fmul_rn(ratio, __fsub_rn(x, old_error))), __fmul_rn(__fadd_rn(x, old_error), gain));
    old_nco = nco;
    old_error = x;
    return nco;
}

// One tracking call of general_work for the epoch at c.epoch_start whose taps are E, P, L.  Fills the record (and the
// dump record, :641-701), advances nitems_read by the new block length; on loss of lock the channel stops (state 0).
__device__ GNSSHIP_LOOP_INLINE void glo_epoch_update(const TrkParams& k, TrkChannel& c, const float* taps, gnsship_trk_epoch& rec,
    gnsship_trk_dump_record* dump)
{
    const double fs = k.conf.fs_in;
    const float* E = taps;
    const float* P = taps + 2;
    const float* L = taps + 4;
    const LoopSet& q = k.ls[0];
    rec.sample_counter = c.epoch_start;
    rec.state = 4;
    rec.flags = 8;
    // PLL (:538-544)
    c.carr_phase_error_hz = pll_error_hz(1, P[0], P[1]);
    c.carr_error_filt_hz = static_cast<double>(glo_filter(c.fp_w, c.fp_x, q.lf_out[0], q.lf_out[1], static_cast<float>(c.carr_phase_error_hz)));
    c.carrier_phase_rate_step_rad += c.carr_error_filt_hz;  // d_carrier_frequency_hz
    c.carrier_doppler_hz += c.carr_error_filt_hz;
    c.code_freq_chips = k.code_chip_rate + (c.carrier_doppler_hz * k.code_chip_rate) / c.code_phase_rate_step_chips;
    // DLL (:548-553): dll_nc_e_minus_l_normalized(E, L, spc, slope 1.0, y_intercept 1.0)
    {
        const double pe = static_cast<double>(hypotf_glibc(E[0], E[1]));
        const double pl = static_cast<double>(hypotf_glibc(L[0], L[1]));
        const double s = pe + pl;
        const float norm = __fdiv_rn(__fsub_rn(1.0f, __fmul_rn(1.0f, k.conf.early_late_space_chips)), 1.0f);
        c.code_error_chips = (s == 0.0) ? 0.0 : static_cast<double>(norm) * (pe - pl) / s;
    }
    c.code_error_filt_chips = static_cast<double>(glo_filter(c.lf_outputs[0], c.lf_inputs[0], q.lf_in[0], q.lf_in[1], static_cast<float>(c.code_error_chips)));
    const double T_chip = 1.0 / c.code_freq_chips;
    const double T_prn = T_chip * static_cast<double>(k.code_length_chips);
    const double code_error_filt_secs = T_prn * c.code_error_filt_chips * T_chip;
    // buffer alignment (:561-563)
    const double T_prn_samples = T_prn * fs;
    c.K_blk_samples = T_prn_samples + c.rem_code_phase_samples + code_error_filt_secs * fs;
    c.current_prn_length_samples = static_cast<int32_t>(round(c.K_blk_samples));
    const double n = static_cast<double>(c.current_prn_length_samples);
    // PLL commands (:567-573)
    const double doppler_phase_step = kTwoPi * c.carrier_doppler_hz / fs;
    c.carrier_phase_step_rad = kTwoPi * c.carrier_phase_rate_step_rad / fs;
    c.rem_carr_phase_rad = __fadd_rn(c.rem_carr_phase_rad, static_cast<float>(c.carrier_phase_step_rad * n));
    c.rem_carr_phase_rad = static_cast<float>(fmod_2pi(static_cast<double>(c.rem_carr_phase_rad)));
    c.acc_carrier_phase_rad -= doppler_phase_step * n;
    // DLL commands (:577-580)
    c.code_phase_step_chips = c.code_freq_chips / fs;
    c.rem_code_phase_samples = c.K_blk_samples - n;
    c.rem_code_phase_chips = c.code_freq_chips * (c.rem_code_phase_samples / fs);
    // CN0 estimation and lock detectors (:583-618)
    bool loss_of_lock = false;
    if (c.cn0_counter < kGloCn0EstimationSamples) {
        c.prompt_buf[2 * c.cn0_counter] = P[0];
        c.prompt_buf[2 * c.cn0_counter + 1] = P[1];
        c.cn0_counter++;
    } else {
        c.cn0_counter = 0;
        c.cn0_db_hz = cn0_m2m4(c.prompt_buf, kGloCn0EstimationSamples, static_cast<float>(k.code_period));
        c.carrier_lock_test = carrier_lock_detector_n(c.prompt_buf, kGloCn0EstimationSamples);
        if (static_cast<double>(c.carrier_lock_test) < k.conf.carrier_lock_th || static_cast<double>(c.cn0_db_hz) < static_cast<double>(k.conf.cn0_min))
            c.carrier_fail++;
        else if (c.carrier_fail > 0)
            c.carrier_fail--;
        if (c.carrier_fail > k.conf.max_carrier_lock_fail) {
            c.carrier_fail = 0;
            c.state = 0;  // d_enable_tracking = false
            loss_of_lock = true;
        }
        if (!c.acc_phase_init) {  // check_carrier_phase_coherent_initialization (:474-482)
            c.acc_carrier_phase_rad = -static_cast<double>(c.rem_carr_phase_rad);
            c.acc_phase_init = 1;
        }
    }
    // the outputs (:620-628)
    rec.prompt_i = static_cast<double>(P[0]);
    rec.prompt_q = static_cast<double>(P[1]);
    rec.flags |= loss_of_lock ? 2 : 1;  // the loss-of-lock event / Flag_valid_symbol_output
    rec.code_phase_samples = c.rem_code_phase_samples;
    rec.carrier_phase_rads = c.acc_carrier_phase_rad;
    rec.carrier_doppler_hz = c.carrier_doppler_hz;
    rec.cn0_db_hz = static_cast<double>(c.cn0_db_hz);
    rec.carrier_lock_test = c.carrier_lock_test;
    rec.code_freq_chips = c.code_freq_chips;
    rec.rem_code_phase_chips = c.rem_code_phase_chips;
    rec.rem_carr_phase_rad = c.rem_carr_phase_rad;
    rec.prn_length_samples = c.current_prn_length_samples;
    if (dump) {  // :641-701: PRN_start_sample_count is d_sample_counter itself; this block has no rate fields
        rec.flags |= 16;
        dump->abs_VE = 0.0f;
        dump->abs_E = hypotf_glibc(E[0], E[1]);
        dump->abs_P = hypotf_glibc(P[0], P[1]);
        dump->abs_L = hypotf_glibc(L[0], L[1]);
        dump->abs_VL = 0.0f;
        dump->prompt_I = P[0];
        dump->prompt_Q = P[1];
        dump->PRN_start_sample_count = c.epoch_start;
        dump->acc_carrier_phase_rad = static_cast<float>(c.acc_carrier_phase_rad);
        dump->carrier_doppler_hz = static_cast<float>(c.carrier_doppler_hz);
        dump->carrier_doppler_rate_hz = 0.0f;
        dump->code_freq_chips = static_cast<float>(c.code_freq_chips);
        dump->code_freq_rate_chips = 0.0f;
        dump->carr_error_hz = static_cast<float>(c.carr_phase_error_hz);
        dump->carr_error_filt_hz = static_cast<float>(c.carr_error_filt_hz);
        dump->code_error_chips = static_cast<float>(c.code_error_chips);
        dump->code_error_filt_chips = static_cast<float>(c.code_error_filt_chips);
        dump->CN0_SNV_dB_Hz = c.cn0_db_hz;
        dump->carrier_lock_test = c.carrier_lock_test;
        dump->aux1 = static_cast<float>(c.rem_code_phase_samples);
        dump->aux2 = static_cast<double>(c.epoch_start + static_cast<uint64_t>(c.current_prn_length_samples));
        dump->PRN = c.prn;
    }
    // consume_each(d_current_prn_length_samples) with the NEW length (:705-707), the IF phase with it
    c.nitems_read = c.epoch_start + static_cast<uint64_t>(c.current_prn_length_samples);
    advance_if(k, c, c.current_prn_length_samples);
}

}  // namespace
}  // namespace gnsship
