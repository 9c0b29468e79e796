// extern "C" access to the reference's Glonass_Gnav_Navigation_Message and Glonass_Gnav_Ephemeris for
// tests/golden/make_gnav_golden.py.  The reference's sources are pulled in by name from the include path the script
// passes; nothing of them is copied here.  The Boost date-time headers they ask for are the script's stand-ins.
#include <gnss_satellite.cc>
#include <glonass_gnav_utc_model.cc>
#include <glonass_gnav_ephemeris.cc>
#include <glonass_gnav_navigation_message.cc>

#include <bitset>
#include <cstdint>
#include <string>

extern "C" {

void* ref_gnav_new() { return new Glonass_Gnav_Navigation_Message(); }

// One string_decoder call on 85 characters '0' / '1', then have_new_ephemeris() and have_new_utc_model() as the telemetry
// block calls them, and the TOW flag cleared as the block clears it.  bits_out: the bitset after CRC_test, bits[0] first.
int32_t ref_gnav_decode(void* h, const char* chars, char* bits_out, int32_t* flags, double* tow, int32_t* wn, double* n)
{
    auto* m = static_cast<Glonass_Gnav_Navigation_Message*>(h);
    const std::string s(chars, 85);
    std::bitset<GLONASS_GNAV_STRING_BITS> b(s);
    m->CRC_test(b);
    for (int i = 0; i < 85; i++) bits_out[i] = b[i] ? '1' : '0';
    const int32_t id = m->string_decoder(s);
    flags[0] = m->get_flag_CRC_test() ? 1 : 0;
    flags[1] = m->is_flag_TOW_set() ? 1 : 0;
    flags[2] = m->get_flag_TOW_new() ? 1 : 0;
    flags[3] = m->have_new_ephemeris() ? 1 : 0;
    flags[4] = m->have_new_utc_model() ? 1 : 0;
    flags[5] = m->get_flag_update_slot_number() ? 1 : 0;
    m->set_flag_update_slot_number(false);
    if (flags[0] && flags[2]) m->set_flag_TOW_new(false);
    const Glonass_Gnav_Ephemeris e = m->get_ephemeris();
    *tow = e.d_TOW;
    *wn = e.d_WN;
    *n = e.d_n;
    return id;
}

void ref_gnav_delete(void* h) { delete static_cast<Glonass_Gnav_Navigation_Message*>(h); }

// glot_to_gpst on an ephemeris with these members
void ref_gnav_glot_to_gpst(double yr, double n_t, double tod_offset, double tau_c, double tau_gps, int32_t* wn, double* tow)
{
    Glonass_Gnav_Ephemeris e;
    e.d_yr = yr;
    e.d_N_T = n_t;
    e.glot_to_gpst(tod_offset, tau_c, tau_gps, wn, tow);
}

// The calendar the above ran on: (y, 1, 1) + add_days at `seconds` of day as days since 6 January 1980 and second of day
void ref_gnav_calendar(int32_t y, int32_t add_days, double seconds, int64_t* day, int64_t* second)
{
    const boost::posix_time::ptime t(boost::gregorian::date(y, 1, 1) + boost::gregorian::days(add_days), boost::posix_time::time_duration(0, 0, seconds));
    *day = (t.date() - boost::gregorian::date(1980, 1, 6)).days();
    *second = t.time_of_day().total_seconds();
}
}
