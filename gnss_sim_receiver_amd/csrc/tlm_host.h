// tlm_host.h — the host half the five telemetry decoders share (tlm_galileo.hip, tlm_gps_lnav.hip, tlm_gps_cnav.hip,
// tlm_bds_dnav.hip, tlm_glo_gnav.hip) beyond what every handle shares (host_api.h: reject, launched, stage, copy_out,
// alloc_all, free_all): the staging buffers of host inputs and the argument checks of the run, channel and state calls.
// A decoder's file keeps its kernels, its Args struct, its launch geometry and what only its family checks.
//
// Every function takes `who`, the entry point's name ("gnsship_dnav_run_symbols"): a rejection's text is "<who>: <what>",
// a HIP error's is "<who>: <HIP's text>", an upload's "<who>(upload): <HIP's text>".  These texts are part of the C ABI
// (tests/test_gpu_tlm_rejections.py).  Order everywhere: argument checks, then set_device, then staging.
// Everything here is `static inline`: the library exports nothing new.
#pragma once
#include "host_api.h"

namespace gnsship {

gnsship_ctx* trk_context(const gnsship_trk* t);  // trk_abi.hip

struct TlmHost {  // what every telemetry handle holds for the calls below
    gnsship_ctx* ctx = nullptr;
    int32_t max_channels = 0, max_rounds = 0;
    DevBuf stage, valid, mask;  // device copies of host inputs: symbols or records; the validity mask; the family's second mask, if any
    // what gnsship_<f>_destroy does ahead of `delete`: wait for the stream, free `owned` and the staging buffers
    void release_all(std::initializer_list<void*> owned)
    {
        quiesce(ctx);
        free_all(owned);
        for (DevBuf* s : {&stage, &valid, &mask}) release(*s);
    }
};

// 0 <= n_rounds <= max_rounds, an input where there is a round (`null_input`: "null symbols" / "null records"), set_device
static inline int tlm_check_run(const TlmHost& h, const char* who, int32_t n_rounds, const void* input, const char* null_input)
{
    if (n_rounds < 0 || n_rounds > h.max_rounds) return reject(h.ctx, GNSSHIP_E_INVAL, who, "0 <= n_rounds <= max_rounds");
    if (n_rounds > 0 && !input) return reject(h.ctx, GNSSHIP_E_INVAL, who, null_input);
    return set_device(h.ctx);
}

// gnsship_<f>_run_symbols up to the launch.  *sym, *valid and *mask (mask: null for a family without a second mask) come
// in as the caller's pointers and leave as device pointers: host arrays go through the staging buffers.
static inline int tlm_symbols_in(TlmHost& h, const char* who, int on_device, int32_t n_rounds, const float** sym, const uint8_t** valid,
    const uint8_t** mask)
{
    if (int rc = tlm_check_run(h, who, n_rounds, *sym, "null symbols")) return rc;
    const size_t n = static_cast<size_t>(n_rounds) * h.max_channels;
    if (on_device || n == 0) return GNSSHIP_OK;
    if (int rc = stage(h.ctx, h.stage, *sym, sizeof(float) * n, who, "upload")) return rc;
    *sym = h.stage.as<float>();
    if (*valid) {
        if (int rc = stage(h.ctx, h.valid, *valid, n, who, "upload")) return rc;
        *valid = h.valid.as<uint8_t>();
    }
    if (mask && *mask) {
        if (int rc = stage(h.ctx, h.mask, *mask, n, who, "upload")) return rc;
        *mask = h.mask.as<uint8_t>();
    }
    return GNSSHIP_OK;
}

// gnsship_<f>_run_records up to the launch.  *rec leaves as a device pointer, null when the run has no round (the kernels
// take a non-null pointer for "records, not floats" and read no entry then).
static inline int tlm_records_in(TlmHost& h, const char* who, int on_device, int32_t n_rounds, const gnsship_trk_epoch** rec)
{
    if (int rc = tlm_check_run(h, who, n_rounds, *rec, "null records")) return rc;
    if (n_rounds == 0) {
        *rec = nullptr;
        return GNSSHIP_OK;
    }
    if (on_device) return GNSSHIP_OK;
    if (int rc = stage(h.ctx, h.stage, *rec, sizeof(gnsship_trk_epoch) * n_rounds * h.max_channels, who, "upload")) return rc;
    *rec = h.stage.as<gnsship_trk_epoch>();
    return GNSSHIP_OK;
}

// gnsship_<f>_run_trk up to the launch: the records the tracker's last run left on the device, in place
static inline int tlm_trk_in(const TlmHost& h, const char* who, gnsship_trk* trk, const gnsship_trk_epoch** rec, int32_t* rounds)
{
    gnsship_ctx* ctx = h.ctx;
    if (!trk) return reject(ctx, GNSSHIP_E_INVAL, who, "null tracking handle");
    if (trk_context(trk) != ctx) return reject(ctx, GNSSHIP_E_INVAL, who, "the tracking handle is on another context");
    int32_t nc = 0;
    if (int rc = gnsship_trk_records_device(trk, rec, rounds, &nc)) {
        if (rc == GNSSHIP_E_STATE) return reject(ctx, GNSSHIP_E_STATE, who, "the tracker's last run kept no records on the device");
        return rc;
    }
    if (nc != h.max_channels) return reject(ctx, GNSSHIP_E_INVAL, who, "the handles' max_channels differ");
    if (*rounds > h.max_rounds) return reject(ctx, GNSSHIP_E_INVAL, who, "the tracker's run had more rounds than max_rounds");
    return set_device(ctx);
}

static inline int tlm_check_channel(const TlmHost& h, const char* who, int32_t channel)
{
    if (channel < 0 || channel >= h.max_channels) return reject(h.ctx, GNSSHIP_E_INVAL, who, "channel out of range");
    return GNSSHIP_OK;
}

// the arguments of gnsship_<f>_state_get and _state_set
static inline int tlm_check_state(const TlmHost& h, const char* who, int32_t channel, const void* st)
{
    if (!st) return reject(h.ctx, GNSSHIP_E_INVAL, who, "null state");
    return tlm_check_channel(h, who, channel);
}

}  // namespace gnsship
