// tests/golden/e5_ref_shim.cc — extern "C" wrappers around the REFERENCE's own Galileo E5a / E5b code
// generators.  make_e5_golden.py compiles this file outside the repository with the reference's libs/
// and core/system_parameters/ directories on the include path and -DHAS_STD_SPAN=1 (the reference's own
// switch); the generator sources are pulled in by name from that include path, never copied.  The one
// GNU Radio header they name (the NCO of complex_exp_gen, which nothing here calls) is a stand-in that
// make_e5_golden.py writes into its scratch directory.
// FIXTURE GENERATION ONLY: the product's generators live in gnss_sim_receiver_amd/csrc/codes.cpp.
#include "gnss_signal_replica.cc"
#include "galileo_e5_signal_replica.cc"

#include <array>
#include <complex>
#include <cstdint>

extern "C" {
static int32_t samples_per_code(int32_t fs) { return static_cast<int32_t>(static_cast<double>(fs) / (10.23e6 / 10230.0)); }
static std::array<char, 3> sig(const char* s) { return {{s[0], s[1], '\0'}}; }

void ref_e5_primary(float* dest, int32_t prn, const char* signal_id)
{
    own::span<std::complex<float>> d(reinterpret_cast<std::complex<float>*>(dest), 10230);
    if (signal_id[0] == '5')
        galileo_e5_a_code_gen_complex_primary(d, prn, sig(signal_id));
    else
        galileo_e5_b_code_gen_complex_primary(d, prn, sig(signal_id));
}

int ref_e5_sampled(float* dest, uint32_t prn, const char* signal_id, int32_t fs, uint32_t chip_shift)
{
    const int32_t n = samples_per_code(fs);
    own::span<std::complex<float>> d(reinterpret_cast<std::complex<float>*>(dest), n);
    if (signal_id[0] == '5')
        galileo_e5_a_code_gen_complex_sampled(d, prn, sig(signal_id), fs, chip_shift);
    else
        galileo_e5_b_code_gen_complex_sampled(d, prn, sig(signal_id), fs, chip_shift);
    return n;
}

const char* ref_e5a_i_secondary() { return GALILEO_E5A_I_SECONDARY_CODE; }
const char* ref_e5b_i_secondary() { return GALILEO_E5B_I_SECONDARY_CODE; }
const char* ref_e5a_q_secondary(int32_t prn) { return GALILEO_E5A_Q_SECONDARY_CODE[prn - 1]; }
const char* ref_e5b_q_secondary(int32_t prn) { return GALILEO_E5B_Q_SECONDARY_CODE[prn - 1]; }
}
