// gnsship_cpp.hpp — header-only C++ mirror of the reference's engine classes, on top of the C ABI
// (include/gnsship.h).  A GNSS-SDR adapter swaps
//   Cpu_Multicorrelator_Real_Codes  → gnsship::Hip_Multicorrelator_Real_Codes
//   pcps_acquisition's FFT core     → gnsship::Pcps_Acquisition_Hip
// keeping method names, argument meaning and the reference's error behaviour (bool returns;
// configuration errors throw std::invalid_argument like Acq_Conf::SetFromConfiguration,
// acq_conf.cc:28-31).  Only the C ABI crosses the shared-library boundary.
#ifndef GNSSHIP_CPP_HPP
#define GNSSHIP_CPP_HPP

#include <algorithm>
#include <array>
#include <cmath>
#include <complex>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gnsship.h"

namespace gnsship {

// One context (device + stream + code bank) per device, shared by every channel of a process.
class Device {
public:
    static std::shared_ptr<Device> get(int device = 0)
    {
        static std::mutex mu;
        static std::map<int, std::weak_ptr<Device>> live;
        std::lock_guard<std::mutex> lk(mu);
        auto sp = live[device].lock();
        if (!sp) {
            sp = std::shared_ptr<Device>(new Device(device));
            live[device] = sp;
        }
        return sp;
    }
    ~Device()
    {
        if (ctx_) gnsship_ctx_destroy(ctx_);
    }
    gnsship_ctx* ctx() const { return ctx_; }
    std::mutex& mutex() { return mu_; }  // serialises calls that share the context stream
    // One C call under the mutex: true when it returns GNSSHIP_OK.  Whoever must hold the lock over more than one call
    // (a create and the error text of its failure, a sequence that must not be interleaved) keeps a guard of its own.
    template <class Fn, class... A>
    bool call(Fn fn, A&&... a)
    {
        std::lock_guard<std::mutex> lk(mu_);
        return fn(std::forward<A>(a)...) == GNSSHIP_OK;
    }

private:
    explicit Device(int device)
    {
        // the library must implement the structs this header was compiled against (gnsship.h ABI notes)
        if (gnsship_abi_version() != GNSSHIP_ABI_VERSION)
            throw std::runtime_error("gnsship: libgnsship ABI " + std::to_string(gnsship_abi_version()) + ", header " +
                                     std::to_string(GNSSHIP_ABI_VERSION));
        if (gnsship_ctx_create(device, &ctx_) != GNSSHIP_OK) throw std::runtime_error("gnsship: no HIP device " + std::to_string(device));
    }
    gnsship_ctx* ctx_ = nullptr;
    std::mutex mu_;
};

// Mirror of Cpu_Multicorrelator_Real_Codes (src/algorithms/tracking/libs/cpu_multicorrelator_real_codes.h:37-61).
class Hip_Multicorrelator_Real_Codes {
public:
    explicit Hip_Multicorrelator_Real_Codes(int device = 0) : dev_(Device::get(device)) {}
    ~Hip_Multicorrelator_Real_Codes() { free(); }
    Hip_Multicorrelator_Real_Codes(const Hip_Multicorrelator_Real_Codes&) = delete;
    Hip_Multicorrelator_Real_Codes& operator=(const Hip_Multicorrelator_Real_Codes&) = delete;

    void set_high_dynamics_resampler(bool use_high_dynamics_resampler)
    {
        high_dyn_ = use_high_dynamics_resampler;
        if (h_) gnsship_corr_set_high_dynamics_resampler(h_, high_dyn_ ? 1 : 0);
    }
    // The volk_gnsssdr rotator variant (GNSSHIP_ROTATOR_*); default AUTO: what the reference's
    // dispatcher runs on this host.  Not part of the reference class (volk chooses there).
    bool set_rotator(int variant)
    {
        rotator_ = variant;
        return !h_ || gnsship_corr_set_rotator(h_, rotator_) == GNSSHIP_OK;
    }
    bool init(int max_signal_length_samples, int n_correlators)
    {
        std::lock_guard<std::mutex> lk(dev_->mutex());
        free_locked();
        n_ = n_correlators;
        if (gnsship_corr_create(dev_->ctx(), max_signal_length_samples, n_correlators, &h_) != GNSSHIP_OK) return false;
        gnsship_corr_set_high_dynamics_resampler(h_, high_dyn_ ? 1 : 0);
        if (gnsship_corr_set_rotator(h_, rotator_) != GNSSHIP_OK) {
            free_locked();
            return false;
        }
        return true;
    }
    // The reference borrows the pointers (:53-63); the device engine copies the code at this call.
    bool set_local_code_and_taps(int code_length_chips, const float* local_code_in, float* shifts_chips)
    {
        return h_ && dev_->call(gnsship_corr_set_local_code_and_taps, h_, code_length_chips, local_code_in, shifts_chips);
    }
    bool set_input_output_vectors(std::complex<float>* corr_out, const std::complex<float>* sig_in)
    {
        out_ = corr_out;
        in_ = sig_in;
        return true;
    }
    bool Carrier_wipeoff_multicorrelator_resampler(float rem_carrier_phase_in_rad, float phase_step_rad, float phase_rate_step_rad,
        float rem_code_phase_chips, float code_phase_step_chips, float code_phase_rate_step_chips, int signal_length_samples)
    {
        if (!h_ || !out_ || !in_) return false;
        std::vector<float> tmp(2 * static_cast<size_t>(n_));
        if (!dev_->call(gnsship_corr_run, h_, in_, GNSSHIP_FMT_CF32, 0, rem_carrier_phase_in_rad, phase_step_rad, phase_rate_step_rad,
                rem_code_phase_chips, code_phase_step_chips, code_phase_rate_step_chips, signal_length_samples, tmp.data()))
            return false;
        for (int t = 0; t < n_; t++) out_[t] = std::complex<float>(tmp[2 * t], tmp[2 * t + 1]);
        return true;
    }
    bool Carrier_wipeoff_multicorrelator_resampler(float rem_carrier_phase_in_rad, float phase_step_rad, float rem_code_phase_chips,
        float code_phase_step_chips, float code_phase_rate_step_chips, int signal_length_samples)
    {
        return Carrier_wipeoff_multicorrelator_resampler(rem_carrier_phase_in_rad, phase_step_rad, 0.0F, rem_code_phase_chips,
            code_phase_step_chips, code_phase_rate_step_chips, signal_length_samples);
    }
    bool free()
    {
        if (h_) dev_->call(gnsship_corr_destroy, h_);
        h_ = nullptr;
        return true;
    }
    const char* last_error() const { return gnsship_last_error(dev_->ctx()); }

private:
    void free_locked()
    {
        if (h_) gnsship_corr_destroy(h_);
        h_ = nullptr;
    }
    std::shared_ptr<Device> dev_;
    gnsship_corr* h_ = nullptr;
    int rotator_ = GNSSHIP_ROTATOR_AUTO;
    int n_ = 0;
    bool high_dyn_ = false;  // Dll_Pll_Conf::high_dyn default (dll_pll_conf.h:80)
    std::complex<float>* out_ = nullptr;
    const std::complex<float>* in_ = nullptr;
};

// Mirror of the Acq_Conf fields the PCPS core reads (src/algorithms/acquisition/libs/acq_conf.h:33-81)
// with SetDerivedParams (acq_conf.cc:113-118).
struct Acq_Conf {
    int64_t fs_in{4000000LL};
    float doppler_step{250.0};
    float pfa{0.0};
    uint32_t sampled_ms{1U};
    uint32_t ms_per_code{1U};
    uint32_t chips_per_second{1023000U};
    uint32_t max_dwells{1U};
    int32_t doppler_max{5000};
    bool bit_transition_flag{false};
    bool use_CFAR_algorithm_flag{true};
    bool make_2_steps{false};
    float doppler_step2{125.0};
    uint32_t num_doppler_bins_step2{4U};
    float pfa2{0.0};
    // acquisition resampler (GNSS-SDR.use_acquisition_resampler): resampled_fs = fs_in when unused
    bool use_automatic_resampler{false};
    int64_t resampled_fs{0LL};
    float resampler_ratio{1.0};
    uint32_t resampler_latency_samples{0U};
    // derived
    float samples_per_ms{0.0};
    float samples_per_code{0.0};
    uint32_t samples_per_chip{2U};
    void SetDerivedParams()
    {
        if (pfa < 0.0F || pfa > 1.0F) pfa = 0.0F;       // acq_conf.cc:63-67
        if (pfa <= 0.0F) use_CFAR_algorithm_flag = false;  // :75-79
        if (pfa2 <= 0.0F || pfa2 > 1.0F) pfa2 = pfa;
        if (resampled_fs == 0) resampled_fs = fs_in;       // SetFromConfiguration (:41)
        samples_per_ms = static_cast<float>(resampled_fs) * 0.001F;
        samples_per_chip = static_cast<unsigned int>(std::ceil(static_cast<float>(resampled_fs) / static_cast<float>(chips_per_second)));
        samples_per_code = samples_per_ms * static_cast<float>(ms_per_code);
    }
    // ConfigureAutomaticResampler (acq_conf.cc:91-107), called by the adapters with the signal's
    // optimum acquisition rate (GPS_L1_CA_OPT_ACQ_FS_SPS = 2e6, ...)
    void ConfigureAutomaticResampler(double opt_freq)
    {
        if (!use_automatic_resampler) return;
        if (static_cast<double>(fs_in) > opt_freq) {
            uint32_t decimation = static_cast<uint32_t>(static_cast<double>(fs_in) / opt_freq);
            while (fs_in % decimation > 0) decimation--;
            resampler_ratio = static_cast<float>(decimation);
            resampled_fs = fs_in / static_cast<int>(resampler_ratio);
        }
        SetDerivedParams();
    }
};

// The acquisition resampler the flowgraph puts in front of a channel's acquisition
// (gnss_flowgraph.cc:1028-1113): decimating low-pass FIR designed for the signal's optimum
// acquisition rate.  Feed it the IF stream; its output is the acquisition's input at resampled_fs;
// latency() is what the flowgraph passes to set_resampler_latency.
class Acq_Resampler_Hip {
public:
    Acq_Resampler_Hip(int64_t fs_in, double opt_acq_fs, int64_t max_in_samples, int device = 0) : dev_(Device::get(device))
    {
        int n = 0;
        if (gnsship_acq_resampler_design(fs_in, opt_acq_fs, &decimation_, nullptr, 0, &n) != GNSSHIP_OK)
            throw std::invalid_argument("gnsship_acq_resampler_design");
        taps_.resize(static_cast<size_t>(n));
        if (n > 0) {
            if (gnsship_acq_resampler_design(fs_in, opt_acq_fs, &decimation_, taps_.data(), n, &n) != GNSSHIP_OK)
                throw std::invalid_argument("gnsship_acq_resampler_design");
            std::lock_guard<std::mutex> lk(dev_->mutex());
            if (gnsship_acq_resampler_create(dev_->ctx(), taps_.data(), n, decimation_, max_in_samples, &h_) != GNSSHIP_OK)
                throw std::invalid_argument(std::string("gnsship_acq_resampler_create: ") + gnsship_last_error(dev_->ctx()));
        }
    }
    ~Acq_Resampler_Hip()
    {
        if (h_) gnsship_acq_resampler_destroy(h_);
    }
    bool enabled() const { return h_ != nullptr; }  // false: "input sampling frequency is too low"
    int decimation() const { return decimation_; }
    uint32_t latency() const { return taps_.empty() ? 0U : static_cast<uint32_t>((taps_.size() - 1) / 2); }
    const std::vector<float>& taps() const { return taps_; }
    // n_in gr_complex samples (a multiple of decimation()) -> n_in / decimation() into out
    bool work(const std::complex<float>* in, int64_t n_in, std::complex<float>* out)
    {
        return h_ && dev_->call(gnsship_acq_resampler_run, h_, in, GNSSHIP_FMT_CF32, 0, n_in, reinterpret_cast<float*>(out), nullptr, nullptr);
    }

private:
    std::shared_ptr<Device> dev_;
    gnsship_acq_resampler* h_ = nullptr;
    int decimation_ = 1;
    std::vector<float> taps_;
};

// The Freq_Xlating_Fir_Filter adapter's configuration (src/algorithms/input_filter/adapters/
// freq_xlating_fir_filter.cc:36-106), property names and defaults as there.  filter_type "lowpass"
// designs firdes::low_pass(1, sampling_frequency, bw, tw) (:99-106; bw = 0 -> (fs / decimation_factor) / 2,
// tw = 0 -> bw / 10); the adapter's other filter types use GNU Radio's pm_remez, which is not restated:
// give their taps explicitly in `taps` (then filter_type is not read).
struct Freq_Xlating_Fir_Filter_Conf {
    double IF{0.0};                          // :41,60
    double sampling_frequency{4000000.0};    // :42,61
    int decimation_factor{1};                // :50,62
    std::string filter_type{"lowpass"};      // the adapter's default "bandpass" needs pm_remez: pass taps
    double bw{0.0};                          // :101-102
    double tw{0.0};                          // :103-104
    std::vector<float> taps;                 // explicit taps_ (:97,105), empty = design by filter_type
    // :37,57: "gr_complex" (freq_xlating_fir_filter_ccf, :111-116), or the real-sampled "float" (_fcf,
    // :118-124), "short" (_scf, :125-131) and "byte" (char_to_short + _scf, :143-150; its factor 256 not applied)
    std::string input_item_type{"gr_complex"};
    // GNSSHIP_FMT_* of input_item_type; -1 for a name the adapter does not know (:160-165)
    int input_format() const
    {
        if (input_item_type == "gr_complex") return GNSSHIP_FMT_CF32;
        if (input_item_type == "float") return GNSSHIP_FMT_RF32;
        if (input_item_type == "short") return GNSSHIP_FMT_RI16;
        if (input_item_type == "byte") return GNSSHIP_FMT_RI8;
        return -1;
    }
};

// The packed file sources' configurations, property names and defaults as in the adapters; format() is the
// GNSSHIP_FMT_PACKED value the signal conditioner reads their byte items with (-1: not a known sample_type).
// Two_Bit_Packed_File_Signal_Source with byte items (two_bit_packed_file_signal_source.cc:33-36,79-91;
// unpack_2bit_samples.cc:150-207).  Short items with big_endian_items are a host byte swap, not mirrored.
struct Two_Bit_Packed_File_Signal_Source_Conf {
    std::string sample_type{"real"};  // "real", "iq", "qi" (:33)
    bool big_endian_bytes{false};     // :35: the first sample of a byte in its most significant bits
    int format() const
    {
        const int order = big_endian_bytes ? GNSSHIP_FMT_PACKED_MSB_FIRST : GNSSHIP_FMT_PACKED_LSB_FIRST;
        if (sample_type == "real") return GNSSHIP_FMT_TWO_BIT_PACKED(GNSSHIP_FMT_PACKED_REAL, order);
        if (sample_type == "iq") return GNSSHIP_FMT_TWO_BIT_PACKED(GNSSHIP_FMT_PACKED_IQ, order);
        if (sample_type == "qi") return GNSSHIP_FMT_TWO_BIT_PACKED(GNSSHIP_FMT_PACKED_QI, order);
        return -1;
    }
};
// Nsr_File_Signal_Source (unpack_byte_2bit_samples.cc:50-65): real, LSB first, the field value itself.
struct Nsr_File_Signal_Source_Conf {
    int format() const { return GNSSHIP_FMT_NSR; }
};
// Two_Bit_Cpx_File_Signal_Source (unpack_byte_2bit_cpx_samples.cc:77-90 + interleaved_short_to_complex(false,
// true), two_bit_cpx_file_signal_source.cc:69; swap = the second short is the real part, restated from GNU
// Radio's published meaning): re = bits 7:6, im = 5:4, then 3:2, 1:0.
struct Two_Bit_Cpx_File_Signal_Source_Conf {
    int format() const { return GNSSHIP_FMT_TWO_BIT_CPX; }
};
// Four_Bit_Cpx_File_Signal_Source (four_bit_cpx_file_signal_source.cc:33-50,108; unpack_byte_4bit_samples.cc:44-65).
struct Four_Bit_Cpx_File_Signal_Source_Conf {
    std::string sample_type{"iq"};  // "iq", "qi" (:33)
    int format() const
    {
        if (sample_type == "iq") return GNSSHIP_FMT_FOUR_BIT_CPX(GNSSHIP_FMT_PACKED_IQ);
        if (sample_type == "qi") return GNSSHIP_FMT_FOUR_BIT_CPX(GNSSHIP_FMT_PACKED_QI);
        return -1;
    }
};

// Mirror of Freq_Xlating_Fir_Filter (freq_xlating_fir_filter.cc; the block of :115,
// gr::filter::freq_xlating_fir_filter_ccf::make(decimation_factor, taps, IF, sampling_frequency)) for up to
// GNSSHIP_COND_MAX_BANDS bands of one input stream — one adapter per band in the reference
// (conf/gnss-sdr_BDS_B3I_GPS_L1_CA_ibyte.conf:41-96), one kernel launch for all of them here.  The output
// stays on the device (dev_out()), where gnsship_acq_run and gnsship_trk_run* consume it in place.
class Freq_Xlating_Fir_Filter_Hip {
public:
    Freq_Xlating_Fir_Filter_Hip(const std::vector<Freq_Xlating_Fir_Filter_Conf>& bands, int64_t max_in_samples, int device = 0)
        : dev_(Device::get(device)), conf_(bands)
    {
        if (bands.empty() || bands.size() > GNSSHIP_COND_MAX_BANDS) throw std::invalid_argument("Freq_Xlating_Fir_Filter_Hip: 1..4 bands");
        std::vector<gnsship_cond_band> cb(bands.size());
        for (size_t b = 0; b < bands.size(); b++) {
            Freq_Xlating_Fir_Filter_Conf& c = conf_[b];
            if (c.sampling_frequency != conf_[0].sampling_frequency || c.input_item_type != conf_[0].input_item_type)
                throw std::invalid_argument("Freq_Xlating_Fir_Filter_Hip: the bands share one input stream (sampling_frequency, input_item_type)");
            if (c.input_format() < 0)
                throw std::invalid_argument("Freq_Xlating_Fir_Filter_Hip: unknown input_item_type " + c.input_item_type);
            if (c.taps.empty()) {
                if (c.filter_type != "lowpass")
                    throw std::invalid_argument("Freq_Xlating_Fir_Filter_Hip: filter_type " + c.filter_type + " needs explicit taps (pm_remez is not restated)");
                int n = 0;
                if (gnsship_cond_lowpass_taps(c.sampling_frequency, c.decimation_factor, c.bw, c.tw, nullptr, 0, &n) != GNSSHIP_OK)
                    throw std::invalid_argument("gnsship_cond_lowpass_taps");
                c.taps.resize(static_cast<size_t>(n));
                if (gnsship_cond_lowpass_taps(c.sampling_frequency, c.decimation_factor, c.bw, c.tw, c.taps.data(), n, &n) != GNSSHIP_OK)
                    throw std::invalid_argument("gnsship_cond_lowpass_taps");
            }
            cb[b] = gnsship_cond_band{c.IF, c.decimation_factor, c.taps.data(), static_cast<int>(c.taps.size())};
        }
        std::lock_guard<std::mutex> lk(dev_->mutex());
        if (gnsship_cond_create(dev_->ctx(), conf_[0].sampling_frequency, cb.data(), static_cast<int>(cb.size()), max_in_samples, &h_) != GNSSHIP_OK)
            throw std::invalid_argument(std::string("gnsship_cond_create: ") + gnsship_last_error(dev_->ctx()));
        dev_out_.assign(cb.size(), nullptr);
        n_out_.assign(cb.size(), 0);
    }
    Freq_Xlating_Fir_Filter_Hip(const Freq_Xlating_Fir_Filter_Conf& band, int64_t max_in_samples, int device = 0)
        : Freq_Xlating_Fir_Filter_Hip(std::vector<Freq_Xlating_Fir_Filter_Conf>{band}, max_in_samples, device)
    {
    }
    ~Freq_Xlating_Fir_Filter_Hip()
    {
        if (h_) gnsship_cond_destroy(h_);
    }
    Freq_Xlating_Fir_Filter_Hip(const Freq_Xlating_Fir_Filter_Hip&) = delete;
    Freq_Xlating_Fir_Filter_Hip& operator=(const Freq_Xlating_Fir_Filter_Hip&) = delete;

    int n_bands() const { return static_cast<int>(conf_.size()); }
    const std::vector<float>& taps(int band = 0) const { return conf_[static_cast<size_t>(band)].taps; }
    int decimation(int band = 0) const { return conf_[static_cast<size_t>(band)].decimation_factor; }
    double output_rate(int band = 0) const { return conf_[static_cast<size_t>(band)].sampling_frequency / decimation(band); }
    // n_in samples in `fmt` (a multiple of every band's decimation_factor), host or device memory.  dev_dst: per-band
    // device destinations (nullptr / nullptr entries = the handle's own buffers, valid until the next work());
    // host_out: per-band host copies (nullptr = none; without one the call is asynchronous on the context stream).
    bool work(const void* in, int fmt, bool in_on_device, int64_t n_in, void* const* dev_dst = nullptr, std::complex<float>* const* host_out = nullptr)
    {
        std::vector<float*> ho(conf_.size(), nullptr);
        if (host_out)
            for (size_t b = 0; b < conf_.size(); b++) ho[b] = reinterpret_cast<float*>(host_out[b]);
        return dev_->call(gnsship_cond_run, h_, in, fmt, in_on_device ? 1 : 0, n_in, dev_dst, host_out ? ho.data() : nullptr, dev_out_.data(), n_out_.data());
    }
    // the same with the items of the configuration's input_item_type (gr_complex / float / short / byte)
    bool work_items(const void* in, bool in_on_device, int64_t n_in, void* const* dev_dst = nullptr, std::complex<float>* const* host_out = nullptr)
    {
        return work(in, conf_[0].input_format(), in_on_device, n_in, dev_dst, host_out);
    }
    int input_format() const { return conf_[0].input_format(); }
    // one band, gr_complex in and out on the host: the adapter's gr_complex -> gr_complex item types (:111-116)
    bool work(const std::complex<float>* in, int64_t n_in, std::complex<float>* out)
    {
        if (conf_.size() != 1) return false;
        std::complex<float>* ho[1] = {out};
        return work(in, GNSSHIP_FMT_CF32, false, n_in, nullptr, ho);
    }
    void* dev_out(int band = 0) const { return dev_out_[static_cast<size_t>(band)]; }
    int64_t n_out(int band = 0) const { return n_out_[static_cast<size_t>(band)]; }
    bool reset(uint64_t first_sample = 0)
    {
        return dev_->call(gnsship_cond_reset, h_, first_sample);
    }
    uint64_t samples_in() const
    {
        uint64_t n = 0;
        gnsship_cond_samples_in(h_, &n);
        return n;
    }
    std::string last_error() const { return gnsship_last_error(dev_->ctx()); }

private:
    std::shared_ptr<Device> dev_;
    std::vector<Freq_Xlating_Fir_Filter_Conf> conf_;
    gnsship_cond* h_ = nullptr;
    std::vector<void*> dev_out_;
    std::vector<int64_t> n_out_;
};

// The configurations of the interference-mitigation adapters, property names and defaults as there.
// Pulse_Blanking_Filter (pulse_blanking_filter.cc:37-80).  |IF| > 1 puts a decimation-1
// freq_xlating_fir_filter_ccf with firdes::low_pass(1, sampling_frequency, bw, tw) in front (:69-80).
struct Pulse_Blanking_Filter_Conf {
    float pfa{0.04F};                       // :39-40
    int length{32};                         // :41-42
    int segments_est{12500};                // :43-44
    int segments_reset{5000000};            // :45-46
    double IF{0.0};                         // :47-49 ("if" / "IF")
    double sampling_frequency{4000000.0};   // :72-73
    double bw{2000000.0};                   // :74-75
    double tw{0.0};                         // :76-77: 0 = bw / 10
    float threshold{0.0F};                  // not a property: > 0 replaces the pfa quantile
};
// Notch_Filter (notch_filter.cc:36-46).
struct Notch_Filter_Conf {
    float pfa{0.001F};
    float p_c_factor{0.9F};
    int length{32};
    int segments_est{12500};
    int segments_reset{5000000};
    float threshold{0.0F};
    int chain_form{GNSSHIP_MIT_CHAIN_AUTO};  // not a property: the device form of the recursion
};
// Notch_Filter_Lite (notch_filter_lite.cc:35-56).  coeff_rate 0 = the adapter's default, sampling_frequency · 0.1.
struct Notch_Filter_Lite_Conf {
    float pfa{0.001F};
    float p_c_factor{0.9F};
    int length{32};
    int segments_est{12500};
    int segments_reset{5000000};
    float sampling_frequency{4000000.0F};  // SignalSource.sampling_frequency (:39,43)
    float coeff_rate{0.0F};                // :44,47
    float threshold{0.0F};
    int chain_form{GNSSHIP_MIT_CHAIN_AUTO};
    // :55-56
    int n_segments_coeff() const
    {
        const float rate = coeff_rate > 0.0F ? coeff_rate : sampling_frequency * 0.1F;
        const int n = static_cast<int>((sampling_frequency / rate) / static_cast<float>(length));
        return std::max(1, n);
    }
};

// Common part of the three mirrors: one gnsship_mit handle.  work() emits the complete segments not yet
// emitted (n_out() samples at dev_out(), and in host_out when given) and keeps the rest on the device.
class Mitigation_Filter_Hip {
public:
    virtual ~Mitigation_Filter_Hip()
    {
        if (h_) gnsship_mit_destroy(h_);
    }
    Mitigation_Filter_Hip(const Mitigation_Filter_Hip&) = delete;
    Mitigation_Filter_Hip& operator=(const Mitigation_Filter_Hip&) = delete;
    // dev_dst: a device buffer of at least pending + n_in samples that does not overlap `in` (nullptr = the handle's
    // own, valid until the next work()); without host_out the call is asynchronous on the context stream.
    virtual bool work(const std::complex<float>* in, bool in_on_device, int64_t n_in, void* dev_dst = nullptr, std::complex<float>* host_out = nullptr)
    {
        return dev_->call(gnsship_mit_run, h_, in, in_on_device ? 1 : 0, n_in, dev_dst, reinterpret_cast<float*>(host_out), &dev_out_, &n_out_);
    }
    void* dev_out() const { return dev_out_; }
    int64_t n_out() const { return n_out_; }
    virtual bool reset()
    {
        return dev_->call(gnsship_mit_reset, h_);
    }
    gnsship_mit_state state() const
    {
        gnsship_mit_state st{};
        dev_->call(gnsship_mit_state_get, h_, &st);
        return st;
    }
    std::string last_error() const { return gnsship_last_error(dev_->ctx()); }

protected:
    Mitigation_Filter_Hip(const gnsship_mit_conf& c, int64_t max_in_samples, int device) : dev_(Device::get(device))
    {
        std::lock_guard<std::mutex> lk(dev_->mutex());
        if (gnsship_mit_create(dev_->ctx(), &c, max_in_samples, &h_) != GNSSHIP_OK)
            throw std::invalid_argument(std::string("gnsship_mit_create: ") + gnsship_last_error(dev_->ctx()));
    }
    std::shared_ptr<Device> dev_;
    gnsship_mit* h_ = nullptr;
    void* dev_out_ = nullptr;
    int64_t n_out_ = 0;
};

// Mirror of Notch_Filter (notch_filter.cc; the block of notch_cc.cc).
class Notch_Filter_Hip : public Mitigation_Filter_Hip {
public:
    explicit Notch_Filter_Hip(const Notch_Filter_Conf& c, int64_t max_in_samples, int device = 0)
        : Mitigation_Filter_Hip(gnsship_mit_conf{GNSSHIP_MIT_NOTCH, c.pfa, c.threshold, c.p_c_factor, c.length, c.segments_est, c.segments_reset, 1, c.chain_form},
              max_in_samples, device)
    {
    }
};

// Mirror of Notch_Filter_Lite (notch_filter_lite.cc; the block of notch_lite_cc.cc).
class Notch_Filter_Lite_Hip : public Mitigation_Filter_Hip {
public:
    explicit Notch_Filter_Lite_Hip(const Notch_Filter_Lite_Conf& c, int64_t max_in_samples, int device = 0)
        : Mitigation_Filter_Hip(gnsship_mit_conf{GNSSHIP_MIT_NOTCH_LITE, c.pfa, c.threshold, c.p_c_factor, c.length, c.segments_est, c.segments_reset,
                                    c.n_segments_coeff(), c.chain_form},
              max_in_samples, device)
    {
    }
};

// Mirror of Pulse_Blanking_Filter (pulse_blanking_filter.cc; the block of pulse_blanking_cc.cc).  With |IF| > 1
// work() first runs the adapter's decimation-1 frequency-translating low-pass on the device (:69-80, :109-118).
class Pulse_Blanking_Filter_Hip : public Mitigation_Filter_Hip {
public:
    explicit Pulse_Blanking_Filter_Hip(const Pulse_Blanking_Filter_Conf& c, int64_t max_in_samples, int device = 0)
        : Mitigation_Filter_Hip(gnsship_mit_conf{GNSSHIP_MIT_PULSE_BLANKING, c.pfa, c.threshold, 0.0F, c.length, c.segments_est, c.segments_reset, 1,
                                    GNSSHIP_MIT_CHAIN_AUTO},
              max_in_samples, device)
    {
        if (std::fabs(c.IF) > 1.0) {
            Freq_Xlating_Fir_Filter_Conf x;
            x.IF = c.IF;
            x.sampling_frequency = c.sampling_frequency;
            x.decimation_factor = 1;
            x.bw = c.bw;
            x.tw = c.tw > 0.0 ? c.tw : c.bw / 10.0;
            xlat_ = std::make_unique<Freq_Xlating_Fir_Filter_Hip>(x, max_in_samples, device);
        }
    }
    bool xlat() const { return static_cast<bool>(xlat_); }
    bool work(const std::complex<float>* in, bool in_on_device, int64_t n_in, void* dev_dst = nullptr, std::complex<float>* host_out = nullptr) override
    {
        if (!xlat_) return Mitigation_Filter_Hip::work(in, in_on_device, n_in, dev_dst, host_out);
        if (n_in == 0) return Mitigation_Filter_Hip::work(in, in_on_device, 0, dev_dst, host_out);
        if (!xlat_->work(in, GNSSHIP_FMT_CF32, in_on_device, n_in)) return false;
        return Mitigation_Filter_Hip::work(static_cast<const std::complex<float>*>(xlat_->dev_out()), true, n_in, dev_dst, host_out);
    }
    bool reset() override
    {
        if (xlat_ && !xlat_->reset()) return false;
        return Mitigation_Filter_Hip::reset();
    }

private:
    std::unique_ptr<Freq_Xlating_Fir_Filter_Hip> xlat_;
};

// Mirror of Viterbi_Decoder (src/algorithms/telemetry_decoder/libs/viterbi_decoder.h:34-57): one object, one
// channel of a gnsship_vit in reference mode, so decode() after decode() carries the 64 path metrics as the
// reference's object does; reset() leaves them alone, as there (viterbi_decoder.cc:123-131 rebuilds the transition
// tables only).  KK and nn other than 7 and 2 throw std::invalid_argument.
class Viterbi_Decoder_Hip {
public:
    Viterbi_Decoder_Hip(int32_t KK, int32_t nn, int32_t LL, const std::array<int32_t, 2>& g, int device = 0) : dev_(Device::get(device)), LL_(LL)
    {
        const gnsship_vit_conf c{KK, nn, {g[0], g[1]}, LL, 0, 0, 0, GNSSHIP_VIT_MODE_REFERENCE};
        std::lock_guard<std::mutex> lk(dev_->mutex());
        if (gnsship_vit_create(dev_->ctx(), &c, 1, &h_) != GNSSHIP_OK)
            throw std::invalid_argument(std::string("gnsship_vit_create: ") + gnsship_last_error(dev_->ctx()));
    }
    ~Viterbi_Decoder_Hip()
    {
        if (h_) gnsship_vit_destroy(h_);
    }
    Viterbi_Decoder_Hip(const Viterbi_Decoder_Hip&) = delete;
    Viterbi_Decoder_Hip& operator=(const Viterbi_Decoder_Hip&) = delete;
    // output_u_int[0 .. LL) = the hard decisions; input_c = 2·(LL + 6) soft symbols (throws std::invalid_argument on
    // other sizes, where the reference would read or write out of bounds)
    void decode(std::vector<int32_t>& output_u_int, const std::vector<float>& input_c)
    {
        if (input_c.size() != static_cast<size_t>(2 * (LL_ + 6)) || output_u_int.size() < static_cast<size_t>(LL_))
            throw std::invalid_argument("Viterbi_Decoder_Hip::decode: 2*(LL + 6) symbols in, LL bits out");
        const int32_t channel = 0;
        bits_.resize(static_cast<size_t>(LL_));
        std::lock_guard<std::mutex> lk(dev_->mutex());
        if (gnsship_vit_run(h_, input_c.data(), 0, 1, &channel, nullptr, bits_.data(), nullptr) != GNSSHIP_OK)
            throw std::runtime_error(std::string("gnsship_vit_run: ") + gnsship_last_error(dev_->ctx()));
        for (int32_t i = 0; i < LL_; i++) output_u_int[static_cast<size_t>(i)] = bits_[static_cast<size_t>(i)];
    }
    void reset() {}
    // d_prev_section
    std::array<float, 64> section() const
    {
        std::array<float, 64> s{};
        dev_->call(gnsship_vit_state_get, h_, 0, s.data());
        return s;
    }

private:
    std::shared_ptr<Device> dev_;
    gnsship_vit* h_ = nullptr;
    int32_t LL_;
    std::vector<uint8_t> bits_;
};

// The page formats of galileo_telemetry_decoder_gs (its constructor, :149-213, and decode_*_word): K = 7, rate 1/2,
// G1 = 171o, G2 = 133o with its output inverted, an 8-row block interleaver and 6 tail bits per frame:
//   I/NAV page part 240 symbols = 8 × 30 → 114 bits, F/NAV page 488 = 8 × 61 → 238, C/NAV page 984 = 8 × 123 → 486.
inline gnsship_vit_conf galileo_vit_conf(int32_t rows, int32_t cols, int mode)
{
    return gnsship_vit_conf{7, 2, {121, 91}, rows * cols / 2 - 6, rows, cols, 1, mode};
}
inline gnsship_vit_conf galileo_inav_vit_conf(int mode = GNSSHIP_VIT_MODE_REFERENCE) { return galileo_vit_conf(8, 30, mode); }
inline gnsship_vit_conf galileo_fnav_vit_conf(int mode = GNSSHIP_VIT_MODE_REFERENCE) { return galileo_vit_conf(8, 61, mode); }
inline gnsship_vit_conf galileo_cnav_vit_conf(int mode = GNSSHIP_VIT_MODE_REFERENCE) { return galileo_vit_conf(8, 123, mode); }

// The first two steps of decode_INAV_word / decode_FNAV_word / decode_CNAV_word for many channels at once: frames as
// received (interleaved, preamble removed) in, data bits out, one Viterbi_Decoder object per channel.
class Galileo_Page_Decoder_Hip {
public:
    Galileo_Page_Decoder_Hip(const gnsship_vit_conf& c, int32_t max_channels, int device = 0) : dev_(Device::get(device)), conf_(c)
    {
        std::lock_guard<std::mutex> lk(dev_->mutex());
        if (gnsship_vit_create(dev_->ctx(), &c, max_channels, &h_) != GNSSHIP_OK)
            throw std::invalid_argument(std::string("gnsship_vit_create: ") + gnsship_last_error(dev_->ctx()));
    }
    ~Galileo_Page_Decoder_Hip()
    {
        if (h_) gnsship_vit_destroy(h_);
    }
    Galileo_Page_Decoder_Hip(const Galileo_Page_Decoder_Hip&) = delete;
    Galileo_Page_Decoder_Hip& operator=(const Galileo_Page_Decoder_Hip&) = delete;
    int32_t frame_symbols() const { return 2 * (conf_.data_length + 6); }
    int32_t data_length() const { return conf_.data_length; }
    // symbols: channels.size() frames of frame_symbols() floats; negate: empty, or one flag per frame (the block's
    // d_flag_PLL_180_deg_phase_locked); bits: resized to channels.size() · data_length() bytes of 0 / 1.  In reference
    // mode a channel may appear once per call.
    bool decode_frames(const std::vector<float>& symbols, const std::vector<int32_t>& channels, const std::vector<uint8_t>& negate,
        std::vector<uint8_t>& bits)
    {
        const size_t n = channels.size();
        if (symbols.size() != n * static_cast<size_t>(frame_symbols()) || (!negate.empty() && negate.size() != n)) return false;
        bits.resize(n * static_cast<size_t>(conf_.data_length));
        return dev_->call(gnsship_vit_run, h_, symbols.data(), 0, static_cast<int32_t>(n), channels.data(), negate.empty() ? nullptr : negate.data(),
            bits.data(), nullptr);
    }
    bool reset_channel(int32_t channel)
    {
        return dev_->call(gnsship_vit_reset_channel, h_, channel);
    }
    std::array<float, 64> section(int32_t channel) const
    {
        std::array<float, 64> s{};
        dev_->call(gnsship_vit_state_get, h_, channel, s.data());
        return s;
    }
    std::string last_error() const { return gnsship_last_error(dev_->ctx()); }

private:
    std::shared_ptr<Device> dev_;
    gnsship_vit_conf conf_;
    gnsship_vit* h_ = nullptr;
};

// What acquisition_core writes into Gnss_Synchro (gnss_synchro.h:52-55; pcps_acquisition.cc:683-696).
struct Acq_Outcome {
    double Acq_delay_samples{0.0};
    double Acq_doppler_hz{0.0};
    uint64_t Acq_samplestamp_samples{0};
    uint32_t Acq_doppler_step{0};
    float test_statistics{0.0F};
    float input_power{0.0F};
    float peak{0.0F};
    bool positive{false};
};

// Regularised lower incomplete gamma P(a, x) for integer a ≥ 1 and its inverse (Newton), the
// boost::math::gamma_p_inv call of pcps_acquisition::calculate_threshold (pcps_acquisition.cc:884-899).
inline double gamma_p_int(int a, double x)
{
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < a; k++) {
        term *= x / k;
        sum += term;
    }
    return 1.0 - std::exp(-x) * sum;
}
inline double gamma_p_inv_int(int a, double p)
{
    if (p <= 0.0) return 0.0;
    if (p >= 1.0) return INFINITY;
    // Q = 1 - p is tiny for CFAR thresholds; iterate on log Q for accuracy.
    const double logq = std::log1p(-p);
    double x = std::max(1.0, a - logq);
    for (int it = 0; it < 100; it++) {
        double term = 1.0, sum = 1.0;
        for (int k = 1; k < a; k++) {
            term *= x / k;
            sum += term;
        }
        const double lq = -x + std::log(sum);  // log Q(a, x)
        double lterm = 1.0;
        for (int k = 1; k < a; k++) lterm *= x / k;  // x^{a-1}/(a-1)!
        const double dlq = -lterm / sum;  // d log Q / dx
        const double step = (lq - logq) / dlq;
        x -= step;
        if (x <= 0.0) x = 1e-12;
        if (std::fabs(step) < 1e-13 * std::max(1.0, x)) break;
    }
    return x;
}

// Mirror of the engine part of pcps_acquisition (pcps_acquisition.cc): set_local_code, init (Doppler
// grid), set_doppler_*, set_threshold, calculate_threshold, acquisition_core over one buffer.
class Pcps_Acquisition_Hip {
public:
    explicit Pcps_Acquisition_Hip(const Acq_Conf& conf, int device = 0) : conf_(conf), dev_(Device::get(device))
    {
        conf_.SetDerivedParams();
        // d_consumed_samples (:71), d_fft_size (:84-91)
        consumed_ = static_cast<int>(conf_.sampled_ms * conf_.samples_per_ms * (conf_.bit_transition_flag ? 2.0 : 1.0));
        fft_size_ = conf_.sampled_ms == conf_.ms_per_code ? consumed_ : 2 * consumed_;
        gnsship_acq_conf c{};
        c.fs_in = conf_.resampled_fs;  // the wipeoff grid runs at the resampled rate (:237)
        c.fft_size = fft_size_;
        c.consumed_samples = consumed_;
        c.bit_transition_flag = conf_.bit_transition_flag ? 1 : 0;
        c.doppler_max = conf_.doppler_max;
        c.doppler_step = static_cast<int32_t>(conf_.doppler_step);
        c.doppler_center = 0;
        c.max_dwells = static_cast<int32_t>(conf_.max_dwells);
        c.use_cfar = conf_.use_CFAR_algorithm_flag ? 1 : 0;
        c.samples_per_chip = static_cast<int32_t>(conf_.samples_per_chip);
        c.samples_per_code = conf_.samples_per_code;
        c.resampler_ratio = conf_.resampler_ratio;
        c.max_prns = 1;
        std::lock_guard<std::mutex> lk(dev_->mutex());
        if (gnsship_acq_create(dev_->ctx(), &c, &h_) != GNSSHIP_OK)
            throw std::invalid_argument(std::string("gnsship_acq_create: ") + gnsship_last_error(dev_->ctx()));
    }
    ~Pcps_Acquisition_Hip()
    {
        if (worker_.joinable()) worker_.join();
        if (h_) gnsship_acq_destroy(h_);
    }
    int fft_size() const { return fft_size_; }
    void set_threshold(float threshold) { threshold_ = threshold; }
    void set_resampler_latency(uint32_t latency_samples) { resampler_latency_ = latency_samples; }  // :168-172
    void set_doppler_max(uint32_t doppler_max) { conf_.doppler_max = static_cast<int32_t>(doppler_max); }
    void set_doppler_step(uint32_t doppler_step) { doppler_step_ = doppler_step; }
    void set_doppler_center(int32_t doppler_center) { doppler_center_ = doppler_center; }
    int consumed_samples() const { return consumed_; }
    // is_fdma() (:211-229) for the satellite this block is to acquire, as set_gnss_synchro + set_local_code leave it:
    // signal "1G" / "2G" gives d_doppler_bias = (int32)(DFRQ · GLONASS_PRN[prn]) and rebuilds the grid with it
    // (update_grid_doppler_wipeoffs adds the bias to every wipeoff frequency, :295-302); any other signal clears the
    // bias.  Acq_doppler_hz is reported without the bias, as the block reports it, and step two of make_2_steps is
    // centred on that reported Doppler (update_grid_doppler_wipeoffs_step2, :305-312, adds no bias).  false: a PRN the
    // GLONASS_PRN table does not hold (the reference's map::at throws there).
    bool set_gnss_synchro(const char* signal, uint32_t prn)
    {
        int32_t bias = 0;
        if (signal && (std::strcmp(signal, "1G") == 0 || std::strcmp(signal, "2G") == 0)) {
            int32_t k = 0;
            if (gnsship_glonass_freq_channel(static_cast<int32_t>(prn), &k) != GNSSHIP_OK) return false;
            bias = static_cast<int32_t>((signal[0] == '1' ? 0.56250e6 : 0.43750e6) * k);
        }
        doppler_bias_ = bias;
        fdma_channels_ = 0;
        return init();
    }
    int32_t doppler_bias() const { return doppler_bias_; }
    // The FDMA sweep (gnsship_acq_set_grid_fdma / gnsship_acq_run_fdma): the one GLONASS code under the grids of several
    // frequency channels in one pass, in place of one block per channel.  init_fdma builds the channel-major grid for
    // the current max / step / center; acquisition_core_fdma runs one dwell and fills one outcome per channel
    // (Acq_doppler_hz without the bias; positive against the threshold).  No step two on this grid.  init() or
    // set_gnss_synchro() returns the block to its own grid.  acquisition_core_fdma searches the code of slot 0 (the
    // block's only one), keeps no grid, and stays outside the block's state machine: it touches neither the dwell
    // counter nor general_work's state, so with max_dwells > 1 successive calls accumulate in the engine until
    // max_dwells is reached and the caller decides when a series ends (init_fdma() or init() restarts it).
    bool init_fdma(const std::vector<int32_t>& bias_hz)
    {
        std::lock_guard<std::mutex> lk(dev_->mutex());
        const int step = doppler_step_ ? static_cast<int>(doppler_step_) : static_cast<int>(conf_.doppler_step);
        if (gnsship_acq_set_grid_fdma(h_, conf_.doppler_max, step, doppler_center_, static_cast<int>(bias_hz.size()), bias_hz.data()) != GNSSHIP_OK)
            return false;
        step_two_ = false;
        fdma_channels_ = static_cast<int>(bias_hz.size());
        calculate_threshold();
        return true;
    }
    bool acquisition_core_fdma(const std::complex<float>* in, uint64_t samp_count, std::vector<Acq_Outcome>& out)
    {
        if (fdma_channels_ < 1) return false;
        std::vector<gnsship_acq_result> r(static_cast<size_t>(fdma_channels_));
        if (!dev_->call(gnsship_acq_run_fdma, h_, in, GNSSHIP_FMT_CF32, 0, 0, r.data(), nullptr)) return false;
        out.assign(r.size(), Acq_Outcome{});
        for (size_t g = 0; g < r.size(); g++) {
            out[g].Acq_delay_samples = r[g].acq_delay_samples - static_cast<double>(resampler_latency_);
            out[g].Acq_doppler_hz = static_cast<double>(r[g].doppler_hz);
            out[g].Acq_samplestamp_samples = static_cast<uint64_t>(std::rint(static_cast<double>(samp_count) * conf_.resampler_ratio));
            out[g].test_statistics = r[g].test_statistic;
            out[g].input_power = r[g].input_power;
            out[g].peak = r[g].peak;
            out[g].positive = r[g].test_statistic > threshold_;
        }
        return true;
    }
    // set_local_code (:175-208): FFT of the zero-padded sampled code + conjugate, on the device
    bool set_local_code(const std::complex<float>* code)
    {
        return dev_->call(gnsship_acq_set_local_code, h_, 0, reinterpret_cast<const float*>(code));
    }
    // init (:248-292): rebuild the Doppler wipeoff grid for the current max/step/center
    bool init()
    {
        std::lock_guard<std::mutex> lk(dev_->mutex());
        const int step = doppler_step_ ? static_cast<int>(doppler_step_) : static_cast<int>(conf_.doppler_step);
        if (gnsship_acq_set_grid(h_, conf_.doppler_max, step, doppler_center_ + doppler_bias_) != GNSSHIP_OK) return false;
        step_two_ = false;
        fdma_channels_ = 0;
        calculate_threshold();
        return true;
    }
    // calculate_threshold (:884-899)
    void calculate_threshold()
    {
        const float pfa = step_two_ ? conf_.pfa2 : conf_.pfa;
        if (pfa <= 0.0F) return;
        int nb = 0;
        gnsship_acq_num_bins(h_, &nb);
        const int effective_fft_size = conf_.bit_transition_flag ? fft_size_ / 2 : fft_size_;
        const int num_bins = effective_fft_size * nb;
        threshold_ = static_cast<float>(2.0 * gamma_p_inv_int(2 * (conf_.bit_transition_flag ? 1 : static_cast<int>(conf_.max_dwells)),
                                                  std::pow(1.0 - pfa, 1.0 / static_cast<float>(num_bins))));
    }
    bool step_two() const { return step_two_; }
    float threshold() const { return threshold_; }
    // acquisition_core (:600-871) over consumed_samples() gr_complex samples (one dwell).  With
    // make_2_steps a step-one detection switches to the narrow step-two grid around its Doppler
    // (:771-787) and reports positive only from step two; a step-two miss returns to step one.
    bool acquisition_core(const std::complex<float>* in, uint64_t samp_count, Acq_Outcome& out)
    {
        gnsship_acq_result r{};
        if (!dev_->call(gnsship_acq_run, h_, in, GNSSHIP_FMT_CF32, 0, 1, &r, nullptr)) return false;
        r.doppler_hz -= doppler_bias_;  // the grid's centre carried the FDMA bias; Acq_doppler_hz does not
        out.Acq_delay_samples = r.acq_delay_samples - static_cast<double>(resampler_latency_);  // :686-687
        out.Acq_doppler_hz = static_cast<double>(r.doppler_hz);
        out.Acq_samplestamp_samples = static_cast<uint64_t>(std::rint(static_cast<double>(samp_count) * conf_.resampler_ratio));  // :689
        out.Acq_doppler_step = step_two_ ? static_cast<uint32_t>(conf_.doppler_step2) : out.Acq_doppler_step;
        out.test_statistics = r.test_statistic;
        if (!step_two_) last_input_power_ = r.input_power;
        out.input_power = step_two_ ? last_input_power_ : r.input_power;
        out.peak = r.peak;
        const bool hit = r.test_statistic > threshold_;
        out.positive = hit && (!conf_.make_2_steps || step_two_);
        if (conf_.make_2_steps) {
            if (hit && !step_two_) {
                if (!dev_->call(gnsship_acq_set_grid_step2, h_, static_cast<float>(r.doppler_hz), conf_.doppler_step2,
                        static_cast<int>(conf_.num_doppler_bins_step2), r.input_power))
                    return false;
                step_two_ = true;
            } else if (step_two_) {
                const int step = doppler_step_ ? static_cast<int>(doppler_step_) : static_cast<int>(conf_.doppler_step);
                if (!dev_->call(gnsship_acq_set_grid, h_, conf_.doppler_max, step, doppler_center_ + doppler_bias_)) return false;
                step_two_ = false;
            }
        }
        calculate_threshold();
        return true;
    }
    const char* last_error() const { return gnsship_last_error(dev_->ctx()); }

    // ---- the block's buffering / decision state machine (general_work :902-1031, blocking mode,
    // with the decision part of acquisition_core :760-864) ----
    enum Acq_Event { ACQ_NONE = 0, ACQ_SUCCESS = 1, ACQ_FAIL = 2 };  // the channel messages (:339-390)
    // set_active (:344-352 of the header) / set_state (:315-336)
    void set_active(bool active) { active_ = active; }
    void set_state(int state)
    {
        fsm_state_ = state;
        if (state == 1) {
            synchro_ = Acq_Outcome{};
            active_ = true;
        }
    }
    bool blocking_on_standby{false};  // Acq_Conf::blocking_on_standby
    // Acq_Conf::blocking (acq_conf.h, default true).  false: state 2 runs acquisition_core in a worker
    // thread that holds the block's lock while it runs (pcps_acquisition.cc:602,1002-1006); general_work
    // returns at once and, while the worker is active, consumes input only when the last dwell is in
    // flight (:918-932).  The worker's decision is reported by the next general_work call.
    bool blocking{true};
    uint64_t sample_counter() const { return sample_counter_; }
    const Acq_Outcome& gnss_synchro() const { return synchro_; }
    bool worker_active() const { return worker_active_; }
    // One general_work call over n gr_complex samples: returns how many it consumed (consume_each)
    // and, when acquisition_core ran and decided, ACQ_SUCCESS / ACQ_FAIL in *event.
    int general_work(const std::complex<float>* in, int n, Acq_Event* event)
    {
        std::unique_lock<std::mutex> lk(set_lock_);  // d_setlock (:917)
        *event = pending_event_;
        pending_event_ = ACQ_NONE;
        if (!active_ || worker_active_) {
            const bool consume = !active_ || (worker_active_ && counter_ == conf_.max_dwells);
            const int c = (!blocking_on_standby && consume) ? n : 0;
            sample_counter_ += static_cast<uint64_t>(c);
            if (step_two_) {
                fsm_state_ = 0;
                active_ = true;
            }
            return c;
        }
        switch (fsm_state_) {
        case 0: {
            synchro_ = Acq_Outcome{};
            fsm_state_ = 1;
            buffer_count_ = 0;
            if (blocking_on_standby) return 0;
            sample_counter_ += static_cast<uint64_t>(n);
            return n;
        }
        case 1: {
            if (buffer_.size() != static_cast<size_t>(consumed_)) buffer_.assign(static_cast<size_t>(consumed_), std::complex<float>{});
            const int inc = (n + buffer_count_ <= consumed_) ? n : consumed_ - buffer_count_;
            std::copy(in, in + inc, buffer_.begin() + buffer_count_);
            if (buffer_count_ >= consumed_) fsm_state_ = 2;  // checked before the increment, as :967-970
            buffer_count_ += inc;
            sample_counter_ += static_cast<uint64_t>(inc);
            return inc;
        }
        default: {
            if (blocking) {
                decide(buffer_.data(), event);
            } else {
                if (worker_.joinable()) worker_.join();  // the previous worker has released the lock
                worker_active_ = true;
                worker_ = std::thread([this]() {
                    std::lock_guard<std::mutex> g(set_lock_);  // acquisition_core holds d_setlock (:602)
                    Acq_Event ev = ACQ_NONE;
                    decide(buffer_.data(), &ev);
                    worker_active_ = false;  // :858
                    pending_event_ = ev;
                });
            }
            buffer_count_ = 0;
            return 0;
        }
        }
    }
    // Wait for a non-blocking acquisition_core in flight (its decision is then pending for the next
    // general_work call).
    void join_worker()
    {
        if (worker_.joinable()) worker_.join();
    }

private:
    // acquisition_core's counter update, core and decision block (:623, :683-696, :760-864)
    void decide(const std::complex<float>* in, Acq_Event* event)
    {
        counter_++;
        gnsship_acq_result r{};
        if (!dev_->call(gnsship_acq_run, h_, in, GNSSHIP_FMT_CF32, 0, 1, &r, nullptr)) return;
        r.doppler_hz -= doppler_bias_;  // the grid's centre carried the FDMA bias; Acq_doppler_hz does not
        synchro_.Acq_delay_samples = r.acq_delay_samples - static_cast<double>(resampler_latency_);
        synchro_.Acq_doppler_hz = static_cast<double>(r.doppler_hz);
        synchro_.Acq_samplestamp_samples = static_cast<uint64_t>(std::rint(static_cast<double>(sample_counter_) * conf_.resampler_ratio));
        synchro_.Acq_doppler_step = step_two_ ? static_cast<uint32_t>(conf_.doppler_step2) : static_cast<uint32_t>(conf_.doppler_step);
        synchro_.test_statistics = r.test_statistic;
        if (!step_two_) last_input_power_ = r.input_power;
        synchro_.input_power = step_two_ ? last_input_power_ : r.input_power;
        synchro_.peak = r.peak;
        bool positive_acq = false;
        const bool hit = r.test_statistic > threshold_;
        auto to_step_one = [&]() {
            const int step = doppler_step_ ? static_cast<int>(doppler_step_) : static_cast<int>(conf_.doppler_step);
            dev_->call(gnsship_acq_set_grid, h_, conf_.doppler_max, step, doppler_center_ + doppler_bias_);
            step_two_ = false;
        };
        auto on_hit = [&]() {
            if (conf_.make_2_steps) {
                if (step_two_) {
                    *event = ACQ_SUCCESS;
                    positive_acq = true;
                    to_step_one();
                    fsm_state_ = 0;
                } else {
                    dev_->call(gnsship_acq_set_grid_step2, h_, static_cast<float>(r.doppler_hz), conf_.doppler_step2,
                        static_cast<int>(conf_.num_doppler_bins_step2), r.input_power);
                    step_two_ = true;
                    counter_ = 0;
                    fsm_state_ = 0;
                }
                calculate_threshold();
            } else {
                *event = ACQ_SUCCESS;
                positive_acq = true;
                fsm_state_ = 0;
            }
        };
        if (!conf_.bit_transition_flag) {
            if (hit) {
                active_ = false;
                on_hit();
            } else {
                fsm_state_ = 1;
            }
            if (counter_ == conf_.max_dwells) {
                if (fsm_state_ != 0) *event = ACQ_FAIL;
                fsm_state_ = 0;
                active_ = false;
                if (step_two_) {
                    to_step_one();
                    calculate_threshold();
                }
            }
        } else {
            active_ = false;
            if (hit) {
                on_hit();
            } else {
                fsm_state_ = 0;
                if (step_two_) {
                    to_step_one();
                    calculate_threshold();
                }
                *event = ACQ_FAIL;
            }
        }
        if (counter_ == conf_.max_dwells || positive_acq || conf_.bit_transition_flag) counter_ = 0;
        if (counter_ == 0) dev_->call(gnsship_acq_reset_dwells, h_);
    }

    std::mutex set_lock_;
    std::thread worker_;
    bool worker_active_ = false;
    Acq_Event pending_event_ = ACQ_NONE;
    bool active_ = false;
    int fsm_state_ = 0;
    int buffer_count_ = 0;
    uint32_t counter_ = 0;
    uint64_t sample_counter_ = 0;
    std::vector<std::complex<float>> buffer_;
    Acq_Outcome synchro_{};
    Acq_Conf conf_;
    std::shared_ptr<Device> dev_;
    gnsship_acq* h_ = nullptr;
    int fft_size_ = 0;
    int consumed_ = 0;
    bool step_two_ = false;
    float last_input_power_ = 0.0F;
    float threshold_ = 0.0F;
    uint32_t doppler_step_ = 0;
    int32_t doppler_center_ = 0;
    int32_t doppler_bias_ = 0;   // d_doppler_bias (is_fdma)
    int fdma_channels_ = 0;      // > 0: the FDMA sweep's grid is set (init_fdma)
    uint32_t resampler_latency_ = 0;
};

// set_local_code of the PCPS acquisition adapters: one sampled code of code_length = floor(fs / codes_per_second) samples
// from gen(dest, fs) (negative: no such code, the result is empty), copied num_codes times into vector_length =
// floor(sampled_ms · samples_per_ms) samples, doubled with bit_transition_flag: the rest stays zero.  fs is the rate the
// acquisition runs at, resampled_fs when set.  The *_acquisition_code functions below are this with their signal's constants.
template <class Gen>
std::vector<std::complex<float>> pcps_acquisition_code(const Acq_Conf& conf, double codes_per_second, uint32_t num_codes, Gen gen)
{
    const int64_t fs = conf.resampled_fs ? conf.resampled_fs : conf.fs_in;
    const auto code_length = static_cast<size_t>(std::floor(static_cast<double>(fs) / codes_per_second));
    const auto vector_length = static_cast<size_t>(std::floor(conf.sampled_ms * (static_cast<float>(fs) * 0.001F)) * (conf.bit_transition_flag ? 2.0 : 1.0));
    std::vector<std::complex<float>> one(code_length), out(std::max(vector_length, code_length * num_codes));
    if (gen(one.data(), static_cast<int32_t>(fs)) < 0) return {};
    for (uint32_t i = 0; i < num_codes; i++) std::copy(one.begin(), one.end(), out.begin() + static_cast<size_t>(i) * code_length);
    return out;
}

// ---- GPS L5 (gps_l5_signal_replica.h, GPS_L5.h:32-46, gps_l5i_pcps_acquisition.cc:49-69, :151-170) ----
constexpr double GPS_L5_FREQ_HZ = 1176.45e6;
constexpr double GPS_L5I_CODE_RATE_CPS = 10.23e6;
constexpr double GPS_L5Q_CODE_RATE_CPS = 10.23e6;
constexpr int32_t GPS_L5I_CODE_LENGTH_CHIPS = 10230;
constexpr int32_t GPS_L5Q_CODE_LENGTH_CHIPS = 10230;
constexpr uint32_t GPS_L5_OPT_ACQ_FS_SPS = 10000000;
// The reference's generators under their names (dest: 10230 floats; sampled: samplesPerCode complex).
// false: PRN outside 1..32 (the reference writes all +1 there).
inline bool gps_l5i_code_gen_float(float* dest, uint32_t prn) { return gnsship_gps_l5i_code_gen_float(dest, static_cast<int32_t>(prn)) == GNSSHIP_OK; }
inline bool gps_l5q_code_gen_float(float* dest, uint32_t prn) { return gnsship_gps_l5q_code_gen_float(dest, static_cast<int32_t>(prn)) == GNSSHIP_OK; }
inline int gps_l5i_code_gen_complex_sampled(std::complex<float>* dest, uint32_t prn, int32_t sampling_freq)
{
    return gnsship_gps_l5i_code_gen_complex_sampled(reinterpret_cast<float*>(dest), prn, sampling_freq);
}
inline int gps_l5q_code_gen_complex_sampled(std::complex<float>* dest, uint32_t prn, int32_t sampling_freq)
{
    return gnsship_gps_l5q_code_gen_complex_sampled(reinterpret_cast<float*>(dest), prn, sampling_freq);
}
// GpsL5iPcpsAcquisition's Acq_Conf: ms_per_code 1, the L5I chip rate, the automatic resampler (when
// conf.use_automatic_resampler) designed for GPS_L5_OPT_ACQ_FS_SPS.  The caller's other fields are kept.
inline Acq_Conf gps_l5i_acq_conf(Acq_Conf conf)
{
    conf.ms_per_code = 1U;
    conf.chips_per_second = static_cast<uint32_t>(GPS_L5I_CODE_RATE_CPS);
    conf.SetDerivedParams();
    conf.ConfigureAutomaticResampler(static_cast<double>(GPS_L5_OPT_ACQ_FS_SPS));
    return conf;
}
// GpsL5iPcpsAcquisition::set_local_code: code_length = floor(resampled_fs / 1000) samples of the sampled
// L5I code, copied sampled_ms times (vector_length = sampled_ms · samples_per_ms, doubled with
// bit_transition_flag: the rest stays zero).  Empty: PRN outside 1..32.
inline std::vector<std::complex<float>> gps_l5i_acquisition_code(uint32_t prn, const Acq_Conf& conf)
{
    return pcps_acquisition_code(conf, GPS_L5I_CODE_RATE_CPS / GPS_L5I_CODE_LENGTH_CHIPS, conf.sampled_ms,
        [prn](std::complex<float>* dest, int32_t fs) { return gps_l5i_code_gen_complex_sampled(dest, prn, fs); });
}

// ---- BeiDou B3I (beidou_b3i_signal_replica.h, Beidou_B3I.h, beidou_b3i_pcps_acquisition.cc:46-63) and GPS L2C,
// the L2 CM code (gps_l2c_signal_replica.h, GPS_L2C.h, gps_l2_m_pcps_acquisition.cc:50-78, :150-170) ----
constexpr double BEIDOU_B3I_FREQ_HZ = 1268.52e6;
constexpr double BEIDOU_B3I_CODE_RATE_CPS = 10.23e6;
constexpr int32_t BEIDOU_B3I_CODE_LENGTH_CHIPS = 10230;
constexpr char BEIDOU_B3I_SECONDARY_CODE_STR[21] = "00000100110101001110";
constexpr char BEIDOU_B3I_GEO_PREAMBLE_SYMBOLS_STR[23] = "1111110000001100001100";
constexpr double GPS_L2_FREQ_HZ = 1227.6e6;
constexpr double GPS_L2_M_CODE_RATE_CPS = 0.5115e6;
constexpr int32_t GPS_L2_M_CODE_LENGTH_CHIPS = 10230;
constexpr uint32_t GPS_L2C_OPT_ACQ_FS_SPS = 2000000;
// The reference's generators under their names (dest: 10230 floats; sampled: samplesPerCode complex).
// false / negative: PRN outside 1..63 (B3I; the reference writes nothing there) or 1..50 (L2 CM; the
// reference writes all +1 there).
inline bool beidou_b3i_code_gen_float(float* dest, int32_t prn, uint32_t chip_shift) { return gnsship_beidou_b3i_code_gen_float(dest, prn, chip_shift) == GNSSHIP_OK; }
inline int beidou_b3i_code_gen_complex_sampled(std::complex<float>* dest, uint32_t prn, int32_t sampling_freq, uint32_t chip_shift)
{
    return gnsship_beidou_b3i_code_gen_complex_sampled(reinterpret_cast<float*>(dest), prn, sampling_freq, chip_shift);
}
inline bool gps_l2c_m_code_gen_float(float* dest, uint32_t prn) { return gnsship_gps_l2c_m_code_gen_float(dest, static_cast<int32_t>(prn)) == GNSSHIP_OK; }
inline int gps_l2c_m_code_gen_complex_sampled(std::complex<float>* dest, uint32_t prn, int32_t sampling_freq)
{
    return gnsship_gps_l2c_m_code_gen_complex_sampled(reinterpret_cast<float*>(dest), prn, sampling_freq);
}
// BeidouB3iPcpsAcquisition's Acq_Conf: ms_per_code 1, the B3I chip rate; its optimum acquisition rate is 100e6,
// so no resampler is ever designed.  The caller's other fields are kept.
inline Acq_Conf beidou_b3i_acq_conf(Acq_Conf conf)
{
    conf.ms_per_code = 1U;
    conf.chips_per_second = static_cast<uint32_t>(BEIDOU_B3I_CODE_RATE_CPS);
    conf.SetDerivedParams();
    conf.ConfigureAutomaticResampler(100e6);
    return conf;
}
// GpsL2MPcpsAcquisition's Acq_Conf: ms_per_code 20 (samples_per_code = samples_per_ms · 20; a sampled_ms that is
// no multiple of 20 becomes 20, acq_conf.cc:48-53), the L2 CM chip rate, the automatic resampler designed for
// GPS_L2C_OPT_ACQ_FS_SPS.
inline Acq_Conf gps_l2_m_acq_conf(Acq_Conf conf)
{
    conf.ms_per_code = 20U;
    if (conf.sampled_ms % 20U != 0U || conf.sampled_ms == 0U) conf.sampled_ms = 20U;
    conf.chips_per_second = static_cast<uint32_t>(GPS_L2_M_CODE_RATE_CPS);
    conf.SetDerivedParams();
    conf.ConfigureAutomaticResampler(static_cast<double>(GPS_L2C_OPT_ACQ_FS_SPS));
    return conf;
}
// set_local_code of the two adapters: code_length = floor(fs / 1000) (B3I) or floor(fs / 50) (L2 CM) samples of
// the sampled code, copied sampled_ms / ms_per_code times into vector_length = floor(sampled_ms · samples_per_ms)
// samples (doubled with bit_transition_flag: the rest stays zero).  Empty: PRN out of range.
inline std::vector<std::complex<float>> acquisition_code_10230(uint32_t prn, const Acq_Conf& conf, bool l2c)
{
    const double rate = l2c ? GPS_L2_M_CODE_RATE_CPS : BEIDOU_B3I_CODE_RATE_CPS;
    return pcps_acquisition_code(conf, rate / 10230.0, conf.sampled_ms / (l2c ? 20U : 1U), [prn, l2c](std::complex<float>* dest, int32_t fs) {
        return l2c ? gps_l2c_m_code_gen_complex_sampled(dest, prn, fs) : beidou_b3i_code_gen_complex_sampled(dest, prn, fs, 0);
    });
}
inline std::vector<std::complex<float>> beidou_b3i_acquisition_code(uint32_t prn, const Acq_Conf& conf) { return acquisition_code_10230(prn, conf, false); }
inline std::vector<std::complex<float>> gps_l2c_m_acquisition_code(uint32_t prn, const Acq_Conf& conf) { return acquisition_code_10230(prn, conf, true); }

// ---- GLONASS L1 / L2 C/A (glonass_l1_signal_replica.h, glonass_l2_signal_replica.h, GLONASS_L1_L2_CA.h, gnss_frequencies.h,
// glonass_l1_ca_pcps_acquisition.cc:49-66 and its L2 twin) ----
constexpr double FREQ1_GLO = 1.60200e9;
constexpr double DFRQ1_GLO = 0.56250e6;
constexpr double FREQ2_GLO = 1.24600e9;
constexpr double DFRQ2_GLO = 0.43750e6;
constexpr double GLONASS_L1_CA_FREQ_HZ = FREQ1_GLO;
constexpr double GLONASS_L1_CA_DFREQ_HZ = DFRQ1_GLO;
constexpr double GLONASS_L1_CA_CODE_RATE_CPS = 0.511e6;
constexpr double GLONASS_L1_CA_CODE_LENGTH_CHIPS = 511.0;
constexpr double GLONASS_L2_CA_FREQ_HZ = FREQ2_GLO;
constexpr double GLONASS_L2_CA_DFREQ_HZ = DFRQ2_GLO;
constexpr double GLONASS_L2_CA_CODE_RATE_CPS = 0.511e6;
constexpr double GLONASS_L2_CA_CODE_LENGTH_CHIPS = 511.0;
// The reference's generators under their names (dest: 511 complex; sampled: (int)(fs / 1000) complex, returns that count).
inline void glonass_l1_ca_code_gen_complex(std::complex<float>* dest, uint32_t chip_shift) { gnsship_glonass_l1_ca_code_gen_complex(reinterpret_cast<float*>(dest), chip_shift); }
inline int glonass_l1_ca_code_gen_complex_sampled(std::complex<float>* dest, int32_t sampling_freq, uint32_t chip_shift)
{
    return gnsship_glonass_l1_ca_code_gen_complex_sampled(reinterpret_cast<float*>(dest), sampling_freq, chip_shift);
}
inline void glonass_l2_ca_code_gen_complex(std::complex<float>* dest, uint32_t chip_shift) { gnsship_glonass_l2_ca_code_gen_complex(reinterpret_cast<float*>(dest), chip_shift); }
inline int glonass_l2_ca_code_gen_complex_sampled(std::complex<float>* dest, int32_t sampling_freq, uint32_t chip_shift)
{
    return gnsship_glonass_l2_ca_code_gen_complex_sampled(reinterpret_cast<float*>(dest), sampling_freq, chip_shift);
}
// GLONASS_PRN.at(prn): the frequency channel of PRN 0..24; false for a PRN the table does not hold.
inline bool glonass_freq_channel(uint32_t prn, int32_t* k) { return gnsship_glonass_freq_channel(static_cast<int32_t>(prn), k) == GNSSHIP_OK; }
// is_fdma()'s d_doppler_bias of a frequency channel: (int32)(DFRQ · k), signal "1G" or "2G"
inline int32_t glonass_doppler_bias_hz(const char* signal, int32_t k) { return static_cast<int32_t>((signal[0] == '1' ? DFRQ1_GLO : DFRQ2_GLO) * k); }
// GlonassL1CaPcpsAcquisition's / GlonassL2CaPcpsAcquisition's Acq_Conf: ms_per_code 1, the C/A chip rate; the optimum
// acquisition rate is 100e6, so no resampler is ever designed.  The caller's other fields are kept.
inline Acq_Conf glonass_l1_ca_acq_conf(Acq_Conf conf)
{
    conf.ms_per_code = 1U;
    conf.chips_per_second = static_cast<uint32_t>(GLONASS_L1_CA_CODE_RATE_CPS);
    conf.SetDerivedParams();
    conf.ConfigureAutomaticResampler(100e6);
    return conf;
}
inline Acq_Conf glonass_l2_ca_acq_conf(Acq_Conf conf) { return glonass_l1_ca_acq_conf(conf); }
// set_local_code of the two adapters: code_length = floor(fs / 1000) samples of the sampled code, copied sampled_ms
// times into vector_length = floor(sampled_ms · samples_per_ms) samples (doubled with bit_transition_flag: the rest zero).
inline std::vector<std::complex<float>> glonass_l1_ca_acquisition_code(const Acq_Conf& conf)
{
    return pcps_acquisition_code(conf, GLONASS_L1_CA_CODE_RATE_CPS / GLONASS_L1_CA_CODE_LENGTH_CHIPS, conf.sampled_ms,
        [](std::complex<float>* dest, int32_t fs) { return glonass_l1_ca_code_gen_complex_sampled(dest, fs, 0); });
}
inline std::vector<std::complex<float>> glonass_l2_ca_acquisition_code(const Acq_Conf& conf) { return glonass_l1_ca_acquisition_code(conf); }

// ---- Galileo E5a / E5b (galileo_e5_signal_replica.h, Galileo_E5a.h, Galileo_E5b.h, galileo_e5a_pcps_acquisition.cc:48-76,
// :145-180 and its E5b twin) ----
constexpr double GALILEO_E5A_FREQ_HZ = 1176.45e6;
constexpr double GALILEO_E5B_FREQ_HZ = 1207.14e6;
constexpr double GALILEO_E5A_CODE_CHIP_RATE_CPS = 10.23e6;
constexpr double GALILEO_E5B_CODE_CHIP_RATE_CPS = 10.23e6;
constexpr int32_t GALILEO_E5A_CODE_LENGTH_CHIPS = 10230;
constexpr int32_t GALILEO_E5B_CODE_LENGTH_CHIPS = 10230;
constexpr int32_t GALILEO_E5A_I_SECONDARY_CODE_LENGTH = 20;
constexpr int32_t GALILEO_E5B_I_SECONDARY_CODE_LENGTH = 4;
constexpr int32_t GALILEO_E5A_Q_SECONDARY_CODE_LENGTH = 100;
constexpr int32_t GALILEO_E5B_Q_SECONDARY_CODE_LENGTH = 100;
constexpr uint32_t GALILEO_E5A_OPT_ACQ_FS_SPS = 10000000;
constexpr uint32_t GALILEO_E5B_OPT_ACQ_FS_SPS = 10000000;
// signal_id "5I" / "5Q" / "5X" ("7I" / "7Q" / "7X"): a single component in the real part, X = I in the real and Q in
// the imaginary part.  false / negative: PRN outside 1..50 or another signal id (the reference writes nothing there).
inline bool galileo_e5_a_code_gen_complex_primary(std::complex<float>* dest, int32_t prn, const std::array<char, 3>& signal_id)
{
    return gnsship_galileo_e5_a_code_gen_complex_primary(reinterpret_cast<float*>(dest), prn, signal_id.data()) == GNSSHIP_OK;
}
inline bool galileo_e5_b_code_gen_complex_primary(std::complex<float>* dest, int32_t prn, const std::array<char, 3>& signal_id)
{
    return gnsship_galileo_e5_b_code_gen_complex_primary(reinterpret_cast<float*>(dest), prn, signal_id.data()) == GNSSHIP_OK;
}
inline int galileo_e5_a_code_gen_complex_sampled(std::complex<float>* dest, uint32_t prn, const std::array<char, 3>& signal_id,
    int32_t sampling_freq, uint32_t chip_shift)
{
    return gnsship_galileo_e5_a_code_gen_complex_sampled(reinterpret_cast<float*>(dest), prn, signal_id.data(), sampling_freq, chip_shift);
}
inline int galileo_e5_b_code_gen_complex_sampled(std::complex<float>* dest, uint32_t prn, const std::array<char, 3>& signal_id,
    int32_t sampling_freq, uint32_t chip_shift)
{
    return gnsship_galileo_e5_b_code_gen_complex_sampled(reinterpret_cast<float*>(dest), prn, signal_id.data(), sampling_freq, chip_shift);
}
// GALILEO_E5A_Q_SECONDARY_CODE[prn − 1] / GALILEO_E5B_Q_SECONDARY_CODE[prn − 1] as a '0' / '1' string; empty: no such
// code (PRN outside 1..50; E5a-Q: outside 1..47, where the reference's table ends)
inline std::string galileo_e5a_q_secondary_code(int32_t prn)
{
    char s[101];
    return gnsship_galileo_e5a_q_secondary_code(s, prn) == GNSSHIP_OK ? std::string(s) : std::string();
}
inline std::string galileo_e5b_q_secondary_code(int32_t prn)
{
    char s[101];
    return gnsship_galileo_e5b_q_secondary_code(s, prn) == GNSSHIP_OK ? std::string(s) : std::string();
}
// GalileoE5aPcpsAcquisition's / GalileoE5bPcpsAcquisition's Acq_Conf: ms_per_code 1, the E5 chip rate, the automatic
// resampler designed for GALILEO_E5A_OPT_ACQ_FS_SPS (E5b's is the same rate).
inline Acq_Conf galileo_e5_acq_conf(Acq_Conf conf)
{
    conf.ms_per_code = 1U;
    conf.chips_per_second = static_cast<uint32_t>(GALILEO_E5A_CODE_CHIP_RATE_CPS);
    conf.SetDerivedParams();
    conf.ConfigureAutomaticResampler(static_cast<double>(GALILEO_E5A_OPT_ACQ_FS_SPS));
    return conf;
}
// set_local_code of the two adapters (:145-180): code_length = floor(fs / 1000) samples of the sampled "5I" code
// ("5Q" with acquire_pilot, "5X" with acquire_iq, which overrides it; band_b: the "7…" codes), copied sampled_ms times.
inline std::vector<std::complex<float>> galileo_e5_acquisition_code(uint32_t prn, const Acq_Conf& conf, bool band_b, bool acquire_pilot = false,
    bool acquire_iq = false)
{
    const std::array<char, 3> id = {{band_b ? '7' : '5', acquire_iq ? 'X' : acquire_pilot ? 'Q' : 'I', '\0'}};
    return pcps_acquisition_code(conf, GALILEO_E5A_CODE_CHIP_RATE_CPS / GALILEO_E5A_CODE_LENGTH_CHIPS, conf.sampled_ms,
        [prn, band_b, &id](std::complex<float>* dest, int32_t fs) {
            return band_b ? galileo_e5_b_code_gen_complex_sampled(dest, prn, id, fs, 0) : galileo_e5_a_code_gen_complex_sampled(dest, prn, id, fs, 0);
        });
}

// Mirror of Dll_Pll_Conf (src/algorithms/tracking/libs/dll_pll_conf.h:33-80): same field names and
// defaults (FLAGS_* defaults from gnss_sdr_flags.cc:48-57 for the lock-detector fields).
struct Dll_Pll_Conf {
    double fs_in{2000000.0};
    double carrier_lock_th{0.7};
    float pll_bw_hz{35.0F}, dll_bw_hz{2.0F}, fll_bw_hz{35.0F};
    float early_late_space_chips{0.25F}, very_early_late_space_chips{0.5F};
    float early_late_space_narrow_chips{0.15F}, very_early_late_space_narrow_chips{0.5F};
    float pll_bw_narrow_hz{5.0F}, dll_bw_narrow_hz{0.75F};
    int32_t extend_correlation_symbols{1};
    bool enable_fll_pull_in{false}, enable_fll_steady_state{false};
    bool high_dyn{false};
    uint32_t smoother_length{10U};
    float slope{1.0F}, spc{0.5F}, y_intercept{1.0F};
    float cn0_smoother_alpha{0.002F}, carrier_lock_test_smoother_alpha{0.002F};
    uint32_t pull_in_time_s{10U}, bit_synchronization_time_limit_s{20U}, vector_length{0U};
    int32_t pll_filter_order{3}, dll_filter_order{2};
    int32_t cn0_samples{20}, cn0_smoother_samples{200}, carrier_lock_test_smoother_samples{25}, cn0_min{25};
    int32_t max_code_lock_fail{50}, max_carrier_lock_fail{5000};
    bool carrier_aiding{true}, track_pilot{true};
    // 'G' GPS (signal "1C": L1 C/A, "L5": the L5Q pilot + L5I prompt, "2S": L2C, the L2 CM code), 'E' Galileo (signal
    // "5X": E5a, "7X": E5b — the Q pilot + the I prompt with track_pilot, the I component alone without — anything else:
    // E1), 'C' BeiDou (signal "B3": B3I, anything else: B1I), 'R' GLONASS (signal "1G": L1 C/A, "2G": L2 C/A — not this
    // block but glonass_l1_ca / glonass_l2_ca_dll_pll_tracking_cc: glonass_l1_ca_trk_conf / glonass_l2_ca_trk_conf below)
    char system{'G'};
    char signal[3]{"1C"};
    // Not a Dll_Pll_Conf member: the reference's correlations follow the volk_gnsssdr rotator variant
    // its dispatcher picks on the host (volk_gnsssdr_rank_archs.c); AUTO makes the same choice.
    int32_t rotator{GNSSHIP_ROTATOR_AUTO};
    // Not a Dll_Pll_Conf member either: InputFilter<i>.IF of the signal's conditioner (the reference removes
    // it ahead of the channels; here the correlator NCO wipes it off, gnsship.h if_hz).
    double if_hz{0.0};
};

// GlonassL1CaDllPllTracking / GlonassL2CaDllPllTracking's configuration (glonass_l1_ca_dll_pll_tracking.cc:44-62): system
// 'R', signal "1G" / "2G", the adapters' defaults pll_bw_hz 50, dll_bw_hz 2, early_late_space_chips 0.5, vector_length =
// round(fs / 1000); max_carrier_lock_fail carries the block's gflag max_lock_fail (50).  The rotator is the generic one:
// the engine has no other for this block (gnsship_trk_create refuses the rest).  The caller's fs_in and if_hz are kept.
inline Dll_Pll_Conf glonass_trk_conf(Dll_Pll_Conf conf, const char* signal)
{
    conf.system = 'R';
    conf.signal[0] = signal[0];
    conf.signal[1] = signal[1];
    conf.signal[2] = '\0';
    conf.pll_bw_hz = 50.0F;
    conf.dll_bw_hz = 2.0F;
    conf.early_late_space_chips = 0.5F;
    conf.max_carrier_lock_fail = 50;
    conf.track_pilot = false;
    conf.rotator = GNSSHIP_ROTATOR_GENERIC;
    conf.vector_length = static_cast<uint32_t>(std::round(conf.fs_in / (0.511e6 / 511.0)));
    return conf;
}
inline Dll_Pll_Conf glonass_l1_ca_trk_conf(const Dll_Pll_Conf& conf) { return glonass_trk_conf(conf, "1G"); }
inline Dll_Pll_Conf glonass_l2_ca_trk_conf(const Dll_Pll_Conf& conf) { return glonass_trk_conf(conf, "2G"); }

// Mirror of dll_pll_veml_tracking (gnuradio_blocks/dll_pll_veml_tracking.cc) for many channels on one
// device: start_tracking(:643-883) per channel, general_work over an IF buffer for all of them (the
// per-epoch loop runs on the device; one record per channel-epoch).
class Dll_Pll_Veml_Tracking_Hip {
public:
    Dll_Pll_Veml_Tracking_Hip(const Dll_Pll_Conf& conf, int max_channels, int device = 0) : dev_(Device::get(device)), channels_(max_channels)
    {
        gnsship_trk_conf c{};
        c.fs_in = conf.fs_in;
        c.carrier_lock_th = conf.carrier_lock_th;
        c.pll_bw_hz = conf.pll_bw_hz;
        c.dll_bw_hz = conf.dll_bw_hz;
        c.fll_bw_hz = conf.fll_bw_hz;
        c.early_late_space_chips = conf.early_late_space_chips;
        c.very_early_late_space_chips = conf.very_early_late_space_chips;
        c.slope = conf.slope;
        c.spc = conf.spc;
        c.y_intercept = conf.y_intercept;
        c.cn0_smoother_alpha = conf.cn0_smoother_alpha;
        c.carrier_lock_test_smoother_alpha = conf.carrier_lock_test_smoother_alpha;
        c.pull_in_time_s = conf.pull_in_time_s;
        c.bit_synchronization_time_limit_s = conf.bit_synchronization_time_limit_s;
        c.vector_length = conf.vector_length;
        c.pll_filter_order = conf.pll_filter_order;
        c.dll_filter_order = conf.dll_filter_order;
        c.cn0_samples = conf.cn0_samples;
        c.cn0_smoother_samples = conf.cn0_smoother_samples;
        c.carrier_lock_test_smoother_samples = conf.carrier_lock_test_smoother_samples;
        c.cn0_min = conf.cn0_min;
        c.max_code_lock_fail = conf.max_code_lock_fail;
        c.max_carrier_lock_fail = conf.max_carrier_lock_fail;
        c.carrier_aiding = conf.carrier_aiding ? 1 : 0;
        c.track_pilot = conf.track_pilot ? 1 : 0;
        c.extend_correlation_symbols = conf.extend_correlation_symbols;
        c.pll_bw_narrow_hz = conf.pll_bw_narrow_hz;
        c.dll_bw_narrow_hz = conf.dll_bw_narrow_hz;
        c.early_late_space_narrow_chips = conf.early_late_space_narrow_chips;
        c.very_early_late_space_narrow_chips = conf.very_early_late_space_narrow_chips;
        c.enable_fll_pull_in = conf.enable_fll_pull_in ? 1 : 0;
        c.enable_fll_steady_state = conf.enable_fll_steady_state ? 1 : 0;
        c.high_dyn = conf.high_dyn ? 1 : 0;
        c.smoother_length = conf.smoother_length;
        c.rotator = conf.rotator;
        c.if_hz = conf.if_hz;
        const bool l5 = conf.system == 'G' && conf.signal[0] == 'L' && conf.signal[1] == '5';  // GpsL5DllPllTracking (system 'G', signal "L5")
        const bool b3 = conf.system == 'C' && conf.signal[0] == 'B' && conf.signal[1] == '3';  // BeidouB3iDllPllTracking
        const bool l2c = conf.system == 'G' && conf.signal[0] == '2' && conf.signal[1] == 'S';  // GpsL2MDllPllTracking
        const bool e5a = conf.system == 'E' && conf.signal[0] == '5' && conf.signal[1] == 'X';  // GalileoE5aDllPllTracking
        const bool e5b = conf.system == 'E' && conf.signal[0] == '7' && conf.signal[1] == 'X';  // GalileoE5bDllPllTracking
        const bool glo = conf.system == 'R' && conf.signal[1] == 'G' && (conf.signal[0] == '1' || conf.signal[0] == '2');  // GlonassL1Ca / L2CaDllPllTracking
        c.system = glo ? (conf.signal[0] == '1' ? GNSSHIP_SYS_GLO_L1CA : GNSSHIP_SYS_GLO_L2CA) : e5a ? GNSSHIP_SYS_GAL_E5A : e5b ? GNSSHIP_SYS_GAL_E5B : conf.system == 'E' ? GNSSHIP_SYS_GAL_E1 : b3 ? GNSSHIP_SYS_BDS_B3I : conf.system == 'C' ? GNSSHIP_SYS_BDS_B1I
                   : l5 ? GNSSHIP_SYS_GPS_L5 : l2c ? GNSSHIP_SYS_GPS_L2C : GNSSHIP_SYS_GPS_L1CA;
        // gps_l5_dll_pll_tracking.cc:49-53 (track_pilot = false — the block's interchange_iq — is refused by gnsship_trk_create)
        if (l5 && c.extend_correlation_symbols < 1) c.extend_correlation_symbols = 1;
        if (b3) {  // beidou_b3i_dll_pll_tracking.cc:47-59
            c.vector_length = static_cast<uint32_t>(std::round(conf.fs_in / (BEIDOU_B3I_CODE_RATE_CPS / BEIDOU_B3I_CODE_LENGTH_CHIPS)));
            c.extend_correlation_symbols = std::min(std::max(c.extend_correlation_symbols, 1), 20);
            c.track_pilot = 0;
        }
        if (e5a || e5b) {  // galileo_e5a_dll_pll_tracking.cc:47-58 and its E5b twin
            c.vector_length = static_cast<uint32_t>(std::round(conf.fs_in / (GALILEO_E5A_CODE_CHIP_RATE_CPS / GALILEO_E5A_CODE_LENGTH_CHIPS)));
            c.extend_correlation_symbols = std::max(c.extend_correlation_symbols, 1);
            if (!c.track_pilot)
                c.extend_correlation_symbols = std::min(c.extend_correlation_symbols,
                    e5a ? GALILEO_E5A_I_SECONDARY_CODE_LENGTH : GALILEO_E5B_I_SECONDARY_CODE_LENGTH);
        }
        if (glo) {  // glonass_l1_ca_dll_pll_tracking.cc:44-62: vector_length alone is derived; the block has no pilot
            c.vector_length = static_cast<uint32_t>(std::round(conf.fs_in / (0.511e6 / 511.0)));
            c.track_pilot = 0;
        }
        if (l2c) {  // gps_l2_m_dll_pll_tracking.cc:47-59: one 20 ms code per epoch, no extension, no pilot
            c.vector_length = static_cast<uint32_t>(std::round(conf.fs_in / (GPS_L2_M_CODE_RATE_CPS / GPS_L2_M_CODE_LENGTH_CHIPS)));
            c.extend_correlation_symbols = 1;
            c.track_pilot = 0;
        }
        glonass_ = glo;
        code_base_ = 1024 + 2 * max_channels * next_engine_id();
        std::lock_guard<std::mutex> lk(dev_->mutex());
        if (gnsship_trk_create(dev_->ctx(), &c, max_channels, &h_) != GNSSHIP_OK)
            throw std::invalid_argument(std::string("gnsship_trk_create: ") + gnsship_last_error(dev_->ctx()));
    }
    ~Dll_Pll_Veml_Tracking_Hip()
    {
        if (h_) gnsship_trk_destroy(h_);
    }
    // start_tracking for one channel: the local code(s) as the block generates them (d_tracking_code,
    // d_data_code; code_len = samples per chip × chips) and the acquisition's Gnss_Synchro fields
    // (prn selects the BeiDou GEO symbol synchronisation and the Galileo E5a / E5b pilot's secondary code).
    bool start_tracking(int channel, const float* tracking_code, const float* data_code, int code_len, double acq_delay_samples,
        double acq_doppler_hz, uint64_t acq_samplestamp_samples, uint64_t first_sample, int prn = 0)
    {
        if (channel < 0 || channel >= channels_) return false;
        std::lock_guard<std::mutex> lk(dev_->mutex());
        const int cid = code_base_ + 2 * channel;
        if (gnsship_code_set(dev_->ctx(), cid, tracking_code, code_len) != GNSSHIP_OK) return false;
        if (data_code && gnsship_code_set(dev_->ctx(), cid + 1, data_code, code_len) != GNSSHIP_OK) return false;
        gnsship_trk_start_args a{};
        a.code_id = cid;
        a.data_code_id = data_code ? cid + 1 : -1;
        a.acq_delay_samples = acq_delay_samples;
        a.acq_doppler_hz = acq_doppler_hz;
        a.acq_samplestamp_samples = acq_samplestamp_samples;
        a.first_sample = first_sample;
        a.prn = prn;
        return gnsship_trk_start(h_, channel, &a) == GNSSHIP_OK;
    }
    bool stop_tracking(int channel)
    {
        return dev_->call(gnsship_trk_stop, h_, channel);
    }
    // msg_handler_telemetry_to_trk (dll_pll_veml_tracking.cc:617-640): the telemetry decoder's
    // fault message (event 1) forces loss of lock at the channel's next lock check
    bool msg_handler_telemetry_to_trk(int channel, int tlm_event)
    {
        return dev_->call(gnsship_trk_telemetry_event, h_, channel, tlm_event);
    }
    // general_work for every channel over gr_complex samples [first_sample, first_sample + n): up to
    // max_epochs epochs per channel; records (max_epochs × max_channels, optional) as gnsship_trk_epoch.
    int work(const std::complex<float>* in, uint64_t first_sample, int64_t n, int max_epochs, gnsship_trk_epoch* records = nullptr,
        bool in_on_device = false)
    {
        int done = 0;
        return dev_->call(gnsship_trk_run, h_, in, GNSSHIP_FMT_CF32, in_on_device ? 1 : 0, first_sample, n, max_epochs, records, &done) ? done : -1;
    }
    // work() with Dll_Pll_Conf::dump on: dumps (max_epochs × max_channels) receives the log_data
    // records (:1376-1466) of the epochs whose record has flags & 16.
    int work_dump(const std::complex<float>* in, uint64_t first_sample, int64_t n, int max_epochs, gnsship_trk_epoch* records,
        gnsship_trk_dump_record* dumps, bool in_on_device = false)
    {
        int done = 0;
        return dev_->call(gnsship_trk_run_dump, h_, in, GNSSHIP_FMT_CF32, in_on_device ? 1 : 0, first_sample, n, max_epochs, records, dumps, &done) ? done : -1;
    }
    // Append channel `channel`'s records to its dump file (<dump_filename><channel>.dat, as the
    // block's d_dump_file): the binary layout tracking_dump_reader reads.
    bool append_dump_file(const std::string& dump_filename, int channel, const gnsship_trk_epoch* records, const gnsship_trk_dump_record* dumps,
        int rounds) const
    {
        const std::string path = dump_filename + std::to_string(channel) + ".dat";
        std::FILE* f = std::fopen(path.c_str(), "ab");
        if (!f) return false;
        bool ok = true;
        for (int r = 0; r < rounds && ok; r++) {
            const size_t i = static_cast<size_t>(r) * channels_ + channel;
            if (!(records[i].flags & 16)) continue;
            if (!glonass_) {
                ok = std::fwrite(&dumps[i], sizeof(gnsship_trk_dump_record), 1, f) == 1;
                continue;
            }
            // glonass_l1_ca_dll_pll_tracking_cc's record (:641-701): 88 bytes, the same without the two rate fields
            const char* d = reinterpret_cast<const char*>(&dumps[i]);
            const size_t r1 = offsetof(gnsship_trk_dump_record, carrier_doppler_rate_hz), c1 = offsetof(gnsship_trk_dump_record, code_freq_chips);
            const size_t r2 = offsetof(gnsship_trk_dump_record, code_freq_rate_chips), c2 = offsetof(gnsship_trk_dump_record, carr_error_hz);
            ok = std::fwrite(d, r1, 1, f) == 1 && std::fwrite(d + c1, r2 - c1, 1, f) == 1 &&
                 std::fwrite(d + c2, sizeof(gnsship_trk_dump_record) - c2, 1, f) == 1;
        }
        return std::fclose(f) == 0 && ok;
    }
    int state(int channel, uint64_t* next_sample = nullptr)
    {
        int st = -1;
        dev_->call(gnsship_trk_channel_state, h_, channel, &st, next_sample);
        return st;
    }
    const char* last_error() const { return gnsship_last_error(dev_->ctx()); }
    gnsship_trk* handle() const { return h_; }  // for Galileo_Telemetry_Decoder_Hip::work_trk
    int channels() const { return channels_; }

private:
    static int next_engine_id()
    {
        static std::atomic<int> n{0};
        return n++;
    }
    std::shared_ptr<Device> dev_;
    gnsship_trk* h_ = nullptr;
    int channels_ = 0;
    int code_base_ = 0;
    bool glonass_ = false;  // the GLONASS block: its dump file has the 88-byte record
};

// ---- The telemetry decoders: five families of blocks (gnsship_tlm_*, _lnav_*, _cnav_*, _dnav_*, _gnav_* of include/gnsship.h),
// each for many channels at once, one block object per channel: symbols or tracking records in, the family's records out. ----

// What the families share, over a family's types and the C functions every family has (the *_Tlm_Api structs below): the
// handle (created and destroyed here, not copyable; deleting a signal-named block through its family class is fine), the
// host vectors a work_* call's outputs land in, sized for the most the C contract lets one run write, state() and
// last_error().  For the family classes: call() and, for the families with a TOW stream, run() / run_trk().
template <class Api>
class Telemetry_Decoder_Hip {
public:
    virtual ~Telemetry_Decoder_Hip()
    {
        if (h_) Api::destroy(h_);
    }
    Telemetry_Decoder_Hip(const Telemetry_Decoder_Hip&) = delete;
    Telemetry_Decoder_Hip& operator=(const Telemetry_Decoder_Hip&) = delete;
    static constexpr bool has_faults = Api::has_faults;  // the family raises faults: it has a public faults()
    const typename Api::Conf& conf() const { return conf_; }
    // the last work_* call's outputs: record k < counts()[c] of channel c is records()[c · per_run() + k] (each family has
    // its own names for the two); entry (r, c), r < rounds(), of a TOW stream is tow_ms()[r · max_channels + c] and
    // sflags()[r · max_channels + c] (Galileo has no stream: empty).  rounds(): n_rounds of work_symbols / work_records;
    // for work_trk 0, then the rounds of the tracker's run as the library reports them
    const std::vector<typename Api::Record>& records() const { return records_; }
    int32_t per_run() const { return per_run_; }
    const std::vector<int32_t>& counts() const { return counts_; }
    const std::vector<uint32_t>& tow_ms() const { return tow_ms_; }
    const std::vector<uint8_t>& sflags() const { return sflags_; }
    int32_t rounds() const { return rounds_; }
    typename Api::State state(int32_t channel) const
    {
        typename Api::State st{};
        call(Api::state_get, channel, &st);
        return st;
    }
    std::string last_error() const { return gnsship_last_error(dev_->ctx()); }

protected:
    Telemetry_Decoder_Hip(const typename Api::Conf& c, int32_t max_channels, int device) : dev_(Device::get(device)), conf_(c)
    {
        std::lock_guard<std::mutex> lk(dev_->mutex());
        if (Api::create(dev_->ctx(), &c, max_channels, &h_) != GNSSHIP_OK)
            throw std::invalid_argument(std::string(Api::create_name) + ": " + gnsship_last_error(dev_->ctx()));
        Api::per_run(h_, &per_run_);
        const size_t nc = static_cast<size_t>(max_channels);
        records_.resize(nc * per_run_);
        counts_.resize(nc);
        if (Api::has_faults) faults_.resize(nc);
        if (Api::has_tow) tow_ms_.resize(nc * c.max_rounds);
        if (Api::has_tow) sflags_.resize(nc * c.max_rounds);
    }
    // for the signal-named block classes: the configuration must be their signal's
    static const typename Api::Conf& require(const typename Api::Conf& c, int32_t signal)
    {
        if (c.signal != signal) throw std::invalid_argument("the configuration's signal is not this block's");
        return c;
    }
    // one C call on the handle, under the device mutex
    template <class Fn, class... A>
    bool call(Fn fn, A... a) const
    {
        return dev_->call(fn, h_, a...);
    }
    // A run of a family with a TOW stream: fn(handle, in..., the host outputs in the C functions' order)
    template <class Fn, class... In>
    bool run(int32_t n_rounds, Fn fn, In... in)
    {
        rounds_ = n_rounds;
        return with_outputs([&](auto... out) { return call(fn, in..., out...); });
    }
    // ... over the records the tracker's last work() left on the device, in place
    template <class Fn>
    bool run_trk(Fn fn, const Dll_Pll_Veml_Tracking_Hip& trk)
    {
        rounds_ = 0;
        return with_outputs([&](auto... out) { return call(fn, trk.handle(), out..., &rounds_); });
    }
    const std::vector<uint8_t>& faults() const { return faults_; }  // public in the families that raise faults

    std::vector<typename Api::Record> records_;
    std::vector<int32_t> counts_;
    std::vector<uint8_t> faults_;

private:
    template <class Use>
    bool with_outputs(Use use)
    {
        if constexpr (Api::has_faults) return use(records_.data(), counts_.data(), faults_.data(), tow_ms_.data(), sflags_.data());
        else return use(records_.data(), counts_.data(), tow_ms_.data(), sflags_.data());
    }
    std::shared_ptr<Device> dev_;
    typename Api::Conf conf_;
    typename Api::Handle* h_ = nullptr;
    int32_t per_run_ = 0, rounds_ = 0;
    std::vector<uint32_t> tow_ms_;
    std::vector<uint8_t> sflags_;
};

// The frame types of galileo_telemetry_decoder_gs (:167-213) as gnsship_tlm_conf: max_rounds is the most symbols per
// channel one work_* call may carry.
inline gnsship_tlm_conf galileo_tlm_conf(int32_t frame_type, int32_t max_rounds, int mode) { return gnsship_tlm_conf{frame_type, mode, max_rounds, 0}; }
inline gnsship_tlm_conf galileo_inav_tlm_conf(int32_t max_rounds, int mode = GNSSHIP_VIT_MODE_REFERENCE) { return galileo_tlm_conf(GNSSHIP_TLM_INAV, max_rounds, mode); }
inline gnsship_tlm_conf galileo_fnav_tlm_conf(int32_t max_rounds, int mode = GNSSHIP_VIT_MODE_REFERENCE) { return galileo_tlm_conf(GNSSHIP_TLM_FNAV, max_rounds, mode); }
inline gnsship_tlm_conf galileo_cnav_tlm_conf(int32_t max_rounds, int mode = GNSSHIP_VIT_MODE_REFERENCE) { return galileo_tlm_conf(GNSSHIP_TLM_CNAV, max_rounds, mode); }

struct Galileo_Tlm_Api {
    using Handle = gnsship_tlm;
    using Conf = gnsship_tlm_conf;
    using Record = gnsship_tlm_page;
    using State = gnsship_tlm_state;
    static constexpr const char* create_name = "gnsship_tlm_create";
    static constexpr auto create = gnsship_tlm_create;
    static constexpr auto destroy = gnsship_tlm_destroy;
    static constexpr auto state_get = gnsship_tlm_state_get;
    static constexpr bool has_faults = true, has_tow = false;
    static void per_run(Handle* h, int32_t* n) { gnsship_tlm_outputs_device(h, nullptr, nullptr, nullptr, nullptr, n); }
};

// The frame handling of galileo_telemetry_decoder_gs::general_work (:872-1094): CRC-checked page parts and
// check_tlm_separation faults out.  After a work_* call, pages() / bits() / counts() / faults() hold that call's outputs.
// The one family without a TOW stream, and the one with a second per-record output, the page's data bits.
class Galileo_Telemetry_Decoder_Hip : public Telemetry_Decoder_Hip<Galileo_Tlm_Api> {
public:
    Galileo_Telemetry_Decoder_Hip(const gnsship_tlm_conf& c, int32_t max_channels, int device = 0)
        : Telemetry_Decoder_Hip(c, max_channels, device),
          data_length_(c.frame_type == GNSSHIP_TLM_INAV ? 114 : c.frame_type == GNSSHIP_TLM_FNAV ? 238 : 486)
    {
        bits_.resize(records_.size() * data_length_);
    }
    int32_t data_length() const { return data_length_; }
    int32_t pages_per_run() const { return per_run(); }
    // the block's set_satellite() (:771-789) and reset() (:792-820) on one channel; new_channel: a new block object
    bool set_satellite(int32_t channel) { return call(gnsship_tlm_set_satellite, channel); }
    bool reset(int32_t channel) { return call(gnsship_tlm_reset_channel, channel); }
    bool new_channel(int32_t channel) { return call(gnsship_tlm_new_channel, channel); }
    // symbols[r · max_channels + c], r < n_rounds; valid: the same shape, or null for all valid
    bool work_symbols(const float* symbols, const uint8_t* valid, int32_t n_rounds, bool on_device = false)
    {
        return call(gnsship_tlm_run_symbols, symbols, valid, on_device ? 1 : 0, n_rounds, records_.data(), bits_.data(), counts_.data(), faults_.data());
    }
    // tracking records of that shape: an entry is a symbol when flags & 1, the symbol is (float)prompt_i
    bool work_records(const gnsship_trk_epoch* records, int32_t n_rounds, bool on_device = false)
    {
        return call(gnsship_tlm_run_records, records, on_device ? 1 : 0, n_rounds, records_.data(), bits_.data(), counts_.data(), faults_.data());
    }
    // the records the tracker's last work() left on the device, in place
    bool work_trk(const Dll_Pll_Veml_Tracking_Hip& trk)
    {
        return call(gnsship_tlm_run_trk, trk.handle(), records_.data(), bits_.data(), counts_.data(), faults_.data());
    }
    // part k < counts()[c] of channel c is pages()[c · pages_per_run() + k], its bits (bytes of 0 / 1) start at
    // bits()[(c · pages_per_run() + k) · data_length()]
    const std::vector<gnsship_tlm_page>& pages() const { return records_; }
    const std::vector<uint8_t>& bits() const { return bits_; }
    using Telemetry_Decoder_Hip::faults;

private:
    int32_t data_length_ = 0;
    std::vector<uint8_t> bits_;
};

// gps_l1_ca_telemetry_decoder_gs as gnsship_lnav_conf: max_rounds is the most entries per channel one work_* call may carry.
inline gnsship_lnav_conf gps_l1_ca_tlm_conf(int32_t max_rounds) { return gnsship_lnav_conf{max_rounds, 0}; }

struct Lnav_Tlm_Api {
    using Handle = gnsship_lnav;
    using Conf = gnsship_lnav_conf;
    using Record = gnsship_lnav_subframe;
    using State = gnsship_lnav_state;
    static constexpr const char* create_name = "gnsship_lnav_create";
    static constexpr auto create = gnsship_lnav_create;
    static constexpr auto destroy = gnsship_lnav_destroy;
    static constexpr auto state_get = gnsship_lnav_state_get;
    static constexpr bool has_faults = true, has_tow = true;
    static void per_run(Handle* h, int32_t* n) { gnsship_lnav_outputs_device(h, nullptr, nullptr, nullptr, nullptr, nullptr, n); }
};

// gps_l1_ca_telemetry_decoder_gs up to the time of week: subframes, the TOW stamp of every entry and check_tlm_separation
// faults out.  After a work_* call, subframes() / counts() / faults() / tow_ms() / sflags() hold that call's outputs.
class Gps_L1_Ca_Telemetry_Decoder_Hip : public Telemetry_Decoder_Hip<Lnav_Tlm_Api> {
public:
    Gps_L1_Ca_Telemetry_Decoder_Hip(const gnsship_lnav_conf& c, int32_t max_channels, int device = 0) : Telemetry_Decoder_Hip(c, max_channels, device) {}
    int32_t subframes_per_run() const { return per_run(); }
    // the block's set_satellite() (:217-224) and reset() (:436-445) on one channel; new_channel: a new block object
    bool set_satellite(int32_t channel) { return call(gnsship_lnav_set_satellite, channel); }
    bool reset(int32_t channel) { return call(gnsship_lnav_reset_channel, channel); }
    bool new_channel(int32_t channel) { return call(gnsship_lnav_new_channel, channel); }
    // symbols[r · max_channels + c], r < n_rounds; valid, flags180: the same shape, or null for all valid / all false
    bool work_symbols(const float* symbols, const uint8_t* valid, const uint8_t* flags180, int32_t n_rounds, bool on_device = false)
    {
        return run(n_rounds, gnsship_lnav_run_symbols, symbols, valid, flags180, on_device ? 1 : 0, n_rounds);
    }
    // tracking records of that shape: a symbol when flags & 1, the symbol is (float)prompt_i, the 180° input flags & 4
    bool work_records(const gnsship_trk_epoch* records, int32_t n_rounds, bool on_device = false)
    {
        return run(n_rounds, gnsship_lnav_run_records, records, on_device ? 1 : 0, n_rounds);
    }
    bool work_trk(const Dll_Pll_Veml_Tracking_Hip& trk) { return run_trk(gnsship_lnav_run_trk, trk); }
    const std::vector<gnsship_lnav_subframe>& subframes() const { return records_; }
    using Telemetry_Decoder_Hip::faults;
};

// gps_l2c_telemetry_decoder_gs / gps_l5_telemetry_decoder_gs as gnsship_cnav_conf: max_rounds is the most entries per
// channel one work_* call may carry.
inline gnsship_cnav_conf gps_l2c_tlm_conf(int32_t max_rounds) { return gnsship_cnav_conf{max_rounds, GNSSHIP_CNAV_L2C, 0}; }
inline gnsship_cnav_conf gps_l5_tlm_conf(int32_t max_rounds) { return gnsship_cnav_conf{max_rounds, GNSSHIP_CNAV_L5, 0}; }

struct Cnav_Tlm_Api {
    using Handle = gnsship_cnav;
    using Conf = gnsship_cnav_conf;
    using Record = gnsship_cnav_message;
    using State = gnsship_cnav_state;
    static constexpr const char* create_name = "gnsship_cnav_create";
    static constexpr auto create = gnsship_cnav_create;
    static constexpr auto destroy = gnsship_cnav_destroy;
    static constexpr auto state_get = gnsship_cnav_state_get;
    static constexpr bool has_faults = true, has_tow = true;
    static void per_run(Handle* h, int32_t* n) { gnsship_cnav_outputs_device(h, nullptr, nullptr, nullptr, nullptr, nullptr, n); }
};

// The GPS CNAV telemetry decoders up to the time of week: messages, the TOW stamp of every entry and watchdog faults out.
// After a work_* call, messages() / counts() / faults() / tow_ms() / sflags() hold that call's outputs.  The two blocks
// differ in the configuration's signal only.
class Gps_Cnav_Telemetry_Decoder_Hip : public Telemetry_Decoder_Hip<Cnav_Tlm_Api> {
public:
    Gps_Cnav_Telemetry_Decoder_Hip(const gnsship_cnav_conf& c, int32_t max_channels, int device = 0) : Telemetry_Decoder_Hip(c, max_channels, device) {}
    int32_t messages_per_run() const { return per_run(); }
    // the block's reset() on one channel; new_channel: a new block object
    bool reset(int32_t channel) { return call(gnsship_cnav_reset_channel, channel); }
    bool new_channel(int32_t channel) { return call(gnsship_cnav_new_channel, channel); }
    // symbols[r · max_channels + c], r < n_rounds; valid, out_valid: the same shape, or null for all valid / all true
    bool work_symbols(const float* symbols, const uint8_t* valid, const uint8_t* out_valid, int32_t n_rounds, bool on_device = false)
    {
        return run(n_rounds, gnsship_cnav_run_symbols, symbols, valid, out_valid, on_device ? 1 : 0, n_rounds);
    }
    // tracking records of that shape: a symbol when flags & 1; the symbol is prompt_i > 0 (L2C) or prompt_q > 0 (L5)
    bool work_records(const gnsship_trk_epoch* records, int32_t n_rounds, bool on_device = false)
    {
        return run(n_rounds, gnsship_cnav_run_records, records, on_device ? 1 : 0, n_rounds);
    }
    bool work_trk(const Dll_Pll_Veml_Tracking_Hip& trk) { return run_trk(gnsship_cnav_run_trk, trk); }
    const std::vector<gnsship_cnav_message>& messages() const { return records_; }
    using Telemetry_Decoder_Hip::faults;
    bool set_state(int32_t channel, const gnsship_cnav_state& st) { return call(gnsship_cnav_state_set, channel, &st); }
};

// gps_l2c_telemetry_decoder_gs: construct with gps_l2c_tlm_conf(max_rounds)
class Gps_L2c_Telemetry_Decoder_Hip : public Gps_Cnav_Telemetry_Decoder_Hip {
public:
    Gps_L2c_Telemetry_Decoder_Hip(const gnsship_cnav_conf& c, int32_t max_channels, int device = 0)
        : Gps_Cnav_Telemetry_Decoder_Hip(require(c, GNSSHIP_CNAV_L2C), max_channels, device) {}
};

// gps_l5_telemetry_decoder_gs: construct with gps_l5_tlm_conf(max_rounds)
class Gps_L5_Telemetry_Decoder_Hip : public Gps_Cnav_Telemetry_Decoder_Hip {
public:
    Gps_L5_Telemetry_Decoder_Hip(const gnsship_cnav_conf& c, int32_t max_channels, int device = 0)
        : Gps_Cnav_Telemetry_Decoder_Hip(require(c, GNSSHIP_CNAV_L5), max_channels, device) {}
};

// beidou_b1i_telemetry_decoder_gs / beidou_b3i_telemetry_decoder_gs as gnsship_dnav_conf: max_rounds is the most entries
// per channel one work_* call may carry.
inline gnsship_dnav_conf beidou_b1i_tlm_conf(int32_t max_rounds) { return gnsship_dnav_conf{max_rounds, GNSSHIP_DNAV_B1I, 0}; }
inline gnsship_dnav_conf beidou_b3i_tlm_conf(int32_t max_rounds) { return gnsship_dnav_conf{max_rounds, GNSSHIP_DNAV_B3I, 0}; }

struct Dnav_Tlm_Api {
    using Handle = gnsship_dnav;
    using Conf = gnsship_dnav_conf;
    using Record = gnsship_dnav_subframe;
    using State = gnsship_dnav_state;
    static constexpr const char* create_name = "gnsship_dnav_create";
    static constexpr auto create = gnsship_dnav_create;
    static constexpr auto destroy = gnsship_dnav_destroy;
    static constexpr auto state_get = gnsship_dnav_state_get;
    static constexpr bool has_faults = false, has_tow = true;
    static void per_run(Handle* h, int32_t* n) { gnsship_dnav_outputs_device(h, nullptr, nullptr, nullptr, nullptr, n); }
};

// The BeiDou D1/D2 telemetry decoders up to the time of week: subframes and the TOW stamp of every entry out; the blocks
// raise no fault.  After a work_* call, subframes() / counts() / tow_ms() / sflags() hold that call's outputs.  The two
// blocks differ in the configuration's signal only: which PRNs take the D2 decoder.
class Beidou_Dnav_Telemetry_Decoder_Hip : public Telemetry_Decoder_Hip<Dnav_Tlm_Api> {
public:
    Beidou_Dnav_Telemetry_Decoder_Hip(const gnsship_dnav_conf& c, int32_t max_channels, int device = 0) : Telemetry_Decoder_Hip(c, max_channels, device) {}
    int32_t subframes_per_run() const { return per_run(); }
    // the block's reset() and set_satellite() on one channel; new_channel: a new block object constructed on this PRN
    bool reset(int32_t channel) { return call(gnsship_dnav_reset_channel, channel); }
    bool set_satellite(int32_t channel, int32_t prn) { return call(gnsship_dnav_set_satellite, channel, prn); }
    bool new_channel(int32_t channel, int32_t prn) { return call(gnsship_dnav_new_channel, channel, prn); }
    // symbols[r · max_channels + c], r < n_rounds; valid, out_valid: the same shape, or null for all valid / all true
    bool work_symbols(const float* symbols, const uint8_t* valid, const uint8_t* out_valid, int32_t n_rounds, bool on_device = false)
    {
        return run(n_rounds, gnsship_dnav_run_symbols, symbols, valid, out_valid, on_device ? 1 : 0, n_rounds);
    }
    // tracking records of that shape: a symbol when flags & 1; the symbol is (float)prompt_i
    bool work_records(const gnsship_trk_epoch* records, int32_t n_rounds, bool on_device = false)
    {
        return run(n_rounds, gnsship_dnav_run_records, records, on_device ? 1 : 0, n_rounds);
    }
    bool work_trk(const Dll_Pll_Veml_Tracking_Hip& trk) { return run_trk(gnsship_dnav_run_trk, trk); }
    const std::vector<gnsship_dnav_subframe>& subframes() const { return records_; }
};

// beidou_b1i_telemetry_decoder_gs: construct with beidou_b1i_tlm_conf(max_rounds)
class Beidou_B1i_Telemetry_Decoder_Hip : public Beidou_Dnav_Telemetry_Decoder_Hip {
public:
    Beidou_B1i_Telemetry_Decoder_Hip(const gnsship_dnav_conf& c, int32_t max_channels, int device = 0)
        : Beidou_Dnav_Telemetry_Decoder_Hip(require(c, GNSSHIP_DNAV_B1I), max_channels, device) {}
};

// beidou_b3i_telemetry_decoder_gs: construct with beidou_b3i_tlm_conf(max_rounds)
class Beidou_B3i_Telemetry_Decoder_Hip : public Beidou_Dnav_Telemetry_Decoder_Hip {
public:
    Beidou_B3i_Telemetry_Decoder_Hip(const gnsship_dnav_conf& c, int32_t max_channels, int device = 0)
        : Beidou_Dnav_Telemetry_Decoder_Hip(require(c, GNSSHIP_DNAV_B3I), max_channels, device) {}
};

// glonass_l1_ca_telemetry_decoder_gs / glonass_l2_ca_telemetry_decoder_gs as gnsship_gnav_conf: max_rounds is the most entries
// per channel one work_* call may carry.
inline gnsship_gnav_conf glonass_l1_ca_tlm_conf(int32_t max_rounds) { return gnsship_gnav_conf{max_rounds, GNSSHIP_GNAV_L1CA, 0}; }
inline gnsship_gnav_conf glonass_l2_ca_tlm_conf(int32_t max_rounds) { return gnsship_gnav_conf{max_rounds, GNSSHIP_GNAV_L2CA, 0}; }

struct Gnav_Tlm_Api {
    using Handle = gnsship_gnav;
    using Conf = gnsship_gnav_conf;
    using Record = gnsship_gnav_string;
    using State = gnsship_gnav_state;
    static constexpr const char* create_name = "gnsship_gnav_create";
    static constexpr auto create = gnsship_gnav_create;
    static constexpr auto destroy = gnsship_gnav_destroy;
    static constexpr auto state_get = gnsship_gnav_state_get;
    static constexpr bool has_faults = false, has_tow = true;
    static void per_run(Handle* h, int32_t* n) { gnsship_gnav_outputs_device(h, nullptr, nullptr, nullptr, nullptr, n); }
};

// The GLONASS GNAV telemetry decoders up to the time of week: decoded strings and the TOW stamp of every entry out; the
// blocks raise no fault and have no reset().  After a work_* call, strings() / counts() / tow_ms() / sflags() hold that
// call's outputs.  The two blocks are one algorithm; the configuration's signal only names the block.
class Glonass_Gnav_Telemetry_Decoder_Hip : public Telemetry_Decoder_Hip<Gnav_Tlm_Api> {
public:
    Glonass_Gnav_Telemetry_Decoder_Hip(const gnsship_gnav_conf& c, int32_t max_channels, int device = 0) : Telemetry_Decoder_Hip(c, max_channels, device) {}
    int32_t strings_per_run() const { return per_run(); }
    // the block's set_satellite() on one channel; new_channel: a new block object constructed on this PRN
    bool set_satellite(int32_t channel, int32_t prn) { return call(gnsship_gnav_set_satellite, channel, prn); }
    bool new_channel(int32_t channel, int32_t prn) { return call(gnsship_gnav_new_channel, channel, prn); }
    // symbols[r · max_channels + c], r < n_rounds; valid: the same shape, or null for all valid; out_valid is not read
    bool work_symbols(const float* symbols, const uint8_t* valid, const uint8_t* out_valid, int32_t n_rounds, bool on_device = false)
    {
        return run(n_rounds, gnsship_gnav_run_symbols, symbols, valid, out_valid, on_device ? 1 : 0, n_rounds);
    }
    // tracking records of that shape: a symbol when flags & 1; the symbol is the record's double prompt_i
    bool work_records(const gnsship_trk_epoch* records, int32_t n_rounds, bool on_device = false)
    {
        return run(n_rounds, gnsship_gnav_run_records, records, on_device ? 1 : 0, n_rounds);
    }
    bool work_trk(const Dll_Pll_Veml_Tracking_Hip& trk) { return run_trk(gnsship_gnav_run_trk, trk); }
    const std::vector<gnsship_gnav_string>& strings() const { return records_; }
    bool set_state(int32_t channel, const gnsship_gnav_state& st) { return call(gnsship_gnav_state_set, channel, &st); }
};

// glonass_l1_ca_telemetry_decoder_gs: construct with glonass_l1_ca_tlm_conf(max_rounds)
class Glonass_L1_Ca_Telemetry_Decoder_Hip : public Glonass_Gnav_Telemetry_Decoder_Hip {
public:
    Glonass_L1_Ca_Telemetry_Decoder_Hip(const gnsship_gnav_conf& c, int32_t max_channels, int device = 0)
        : Glonass_Gnav_Telemetry_Decoder_Hip(require(c, GNSSHIP_GNAV_L1CA), max_channels, device) {}
};

// glonass_l2_ca_telemetry_decoder_gs: construct with glonass_l2_ca_tlm_conf(max_rounds)
class Glonass_L2_Ca_Telemetry_Decoder_Hip : public Glonass_Gnav_Telemetry_Decoder_Hip {
public:
    Glonass_L2_Ca_Telemetry_Decoder_Hip(const gnsship_gnav_conf& c, int32_t max_channels, int device = 0)
        : Glonass_Gnav_Telemetry_Decoder_Hip(require(c, GNSSHIP_GNAV_L2CA), max_channels, device) {}
};

}  // namespace gnsship

#endif  // GNSSHIP_CPP_HPP
