// tests/golden/b3i_l2c_ref_shim.cc — extern "C" wrappers around the REFERENCE's own BeiDou B3I and GPS L2C
// (L2 CM) code generators.  make_b3i_l2c_golden.py compiles this file outside the repository with the
// reference's libs/ and core/system_parameters/ directories on the include path and -DHAS_STD_SPAN=1 (the
// reference's own switch); the generator sources are pulled in by name from that include path, never copied.
// FIXTURE GENERATION ONLY: the product's generators live in gnss_sim_receiver_amd/csrc/codes.cpp.
#include "beidou_b3i_signal_replica.cc"
#include "gps_l2c_signal_replica.cc"

#include <complex>
#include <cstdint>

extern "C" {
void ref_beidou_b3i_code_gen_float(float* dest, int32_t prn, uint32_t chip_shift)
{
    beidou_b3i_code_gen_float(own::span<float>(dest, 10230), prn, chip_shift);
}
void ref_gps_l2c_m_code_gen_float(float* dest, uint32_t prn) { gps_l2c_m_code_gen_float(own::span<float>(dest, 10230), prn); }
static int32_t samples_per_code(int32_t fs, double chip_rate) { return static_cast<int32_t>(static_cast<double>(fs) / (chip_rate / 10230.0)); }
int ref_beidou_b3i_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs, uint32_t chip_shift)
{
    const int32_t n = samples_per_code(fs, 10.23e6);
    beidou_b3i_code_gen_complex_sampled(own::span<std::complex<float>>(reinterpret_cast<std::complex<float>*>(dest), n), prn, fs, chip_shift);
    return n;
}
int ref_gps_l2c_m_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs)
{
    const int32_t n = samples_per_code(fs, 0.5115e6);
    gps_l2c_m_code_gen_complex_sampled(own::span<std::complex<float>>(reinterpret_cast<std::complex<float>*>(dest), n), prn, fs);
    return n;
}
}
