// extern "C" access to the reference's Beidou_Dnav_Navigation_Message for tests/golden/make_dnav_golden.py.  The
// reference's sources are pulled in by name from the include path the script passes; nothing of them is copied here.
#include <gnss_satellite.cc>
#include <beidou_dnav_ephemeris.cc>
#include <beidou_dnav_navigation_message.cc>

#include <cstdint>
#include <string>

extern "C" {

void* ref_dnav_new() { return new Beidou_Dnav_Navigation_Message(); }

// one d1_subframe_decoder (d2 == 0) or d2_subframe_decoder call on 300 characters '0' / '1', as the telemetry block makes
// them: the returned ID; get_SOW(), the CRC flag and the new-SOW flag after it.  The flag is then cleared, as the block does.
int32_t ref_dnav_decode(void* h, int32_t d2, const char* bits, double* sow, int32_t* crc, int32_t* new_sow)
{
    auto* m = static_cast<Beidou_Dnav_Navigation_Message*>(h);
    const std::string s(bits, 300);
    const int32_t id = d2 ? m->d2_subframe_decoder(s) : m->d1_subframe_decoder(s);
    *sow = m->get_SOW();
    *crc = m->get_flag_CRC_test() ? 1 : 0;
    *new_sow = m->get_flag_new_SOW_available() ? 1 : 0;
    m->set_flag_new_SOW_available(false);
    return id;
}

void ref_dnav_delete(void* h) { delete static_cast<Beidou_Dnav_Navigation_Message*>(h); }
}
