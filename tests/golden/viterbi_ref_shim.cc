// tests/golden/viterbi_ref_shim.cc — extern "C" wrappers around the REFERENCE's own Viterbi_Decoder
// (telemetry_decoder/libs/viterbi_decoder.cc).  make_viterbi_golden.py compiles this file outside the
// repository with the reference's telemetry_decoder/libs/ directory on the include path; the source is pulled in
// by name from there, never copied.  Its one outside call, volk_gnsssdr_32f_index_max_32u, is declared by a
// one-line <volk_gnsssdr/volk_gnsssdr.h> the script writes into the scratch directory and defined there from the
// reference's _generic kernel header.  `private` is opened after the standard headers so that the fixture also
// holds d_prev_section, the 64 metrics an object carries from one decode() to the next.
// FIXTURE GENERATION ONLY: the product's decoder lives in gnss_sim_receiver_amd/csrc/vit_decoder.hip.
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <vector>

#define private public
#include "viterbi_decoder.cc"
#undef private

extern "C" {
void* ref_vit_new(int32_t KK, int32_t nn, int32_t LL, int32_t g0, int32_t g1)
{
    return new Viterbi_Decoder(KK, nn, LL, std::array<int32_t, 2>{g0, g1});
}

// one decode() of 2·(LL + 6) symbols: LL bits, then the object's 64 carried metrics
void ref_vit_decode(void* h, const float* in, int32_t n_in, int32_t* bits, int32_t LL, float* section)
{
    auto* d = static_cast<Viterbi_Decoder*>(h);
    const std::vector<float> input(in, in + n_in);
    std::vector<int32_t> out(LL);
    d->decode(out, input);
    std::memcpy(bits, out.data(), sizeof(int32_t) * LL);
    std::memcpy(section, d->d_prev_section.data(), sizeof(float) * 64);
}

void ref_vit_reset(void* h) { static_cast<Viterbi_Decoder*>(h)->reset(); }

void ref_vit_delete(void* h) { delete static_cast<Viterbi_Decoder*>(h); }
}
