// extern "C" access to the reference's Gps_Navigation_Message for tests/golden/make_lnav_golden.py.  The reference's
// sources are pulled in by name from the include path the script passes; nothing of them is copied here.
#include <gnss_satellite.cc>
#include <gps_ephemeris.cc>
#include <gps_navigation_message.cc>

#include <cstdint>

extern "C" {

void* ref_lnav_new() { return new Gps_Navigation_Message(); }

// one subframe_decoder call on 40 bytes (ten words as the telemetry block stores them): the returned ID, and get_TOW() after it
int32_t ref_lnav_decode(void* h, const char* subframe, int32_t* tow)
{
    auto* m = static_cast<Gps_Navigation_Message*>(h);
    const int32_t id = m->subframe_decoder(subframe);
    *tow = m->get_TOW();
    return id;
}

void ref_lnav_delete(void* h) { delete static_cast<Gps_Navigation_Message*>(h); }
}
