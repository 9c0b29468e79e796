// tests/golden/l5_ref_shim.cc — extern "C" wrappers around the REFERENCE's own GPS L5 code generators.
// make_l5_golden.py compiles this file outside the repository with the reference's libs/ and
// core/system_parameters/ directories on the include path and -DHAS_STD_SPAN=1 (the reference's own
// switch); the generator source is pulled in by name from that include path, never copied.
// FIXTURE GENERATION ONLY: the product's generators live in gnss_sim_receiver_amd/csrc/codes.cpp.
#include "gps_l5_signal_replica.cc"

#include <complex>
#include <cstdint>

extern "C" {
void ref_gps_l5i_code_gen_float(float* dest, uint32_t prn) { gps_l5i_code_gen_float(own::span<float>(dest, 10230), prn); }
void ref_gps_l5q_code_gen_float(float* dest, uint32_t prn) { gps_l5q_code_gen_float(own::span<float>(dest, 10230), prn); }
static int32_t samples_per_code(int32_t fs) { return static_cast<int32_t>(static_cast<double>(fs) / (10.23e6 / 10230.0)); }
int ref_gps_l5i_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs)
{
    const int32_t n = samples_per_code(fs);
    gps_l5i_code_gen_complex_sampled(own::span<std::complex<float>>(reinterpret_cast<std::complex<float>*>(dest), n), prn, fs);
    return n;
}
int ref_gps_l5q_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs)
{
    const int32_t n = samples_per_code(fs);
    gps_l5q_code_gen_complex_sampled(own::span<std::complex<float>>(reinterpret_cast<std::complex<float>*>(dest), n), prn, fs);
    return n;
}
}
