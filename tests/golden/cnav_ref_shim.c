/* cnav_ref_shim.c — what tests/golden/make_cnav_golden.py loads to record the reference's libswiftcnav at work.  This
 * file is the project's own text: it includes the library's public header and is linked with the library's four source
 * files (cnav_msg.c, viterbi27.c, bits.c, edc.c), which make_cnav_golden.py names on the compile line from the reference
 * tree as separate translation units (viterbi27.c and bits.c both define `parity`).  Nothing of the library is copied. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "cnav_msg.h"

void* ref_cnav_new(void)
{
    cnav_msg_decoder_t* d = (cnav_msg_decoder_t*)malloc(sizeof(cnav_msg_decoder_t));
    if (d) cnav_msg_decoder_init(d);
    return d;
}

void ref_cnav_delete(void* h) { free(h); }

/* Every metric of both buffers of both parts grows by `bias` (modulo 2^32): a state just under the normalisation limit. */
void ref_cnav_add_metrics(void* h, uint32_t bias)
{
    cnav_msg_decoder_t* d = (cnav_msg_decoder_t*)h;
    cnav_v27_part_t* parts[2] = {&d->part1, &d->part2};
    for (int k = 0; k < 2; k++)
        for (int i = 0; i < 64; i++) {
            parts[k]->dec.metrics1[i] += bias;
            parts[k]->dec.metrics2[i] += bias;
        }
}

/* One symbol.  Returns the library's verdict; on true out5 = delay, tow, msg_id, prn, alert and raw64 the raw message. */
int32_t ref_cnav_add_symbol(void* h, uint8_t symbol, uint32_t* out5, uint8_t* raw64)
{
    cnav_msg_t msg;
    uint32_t delay = 0;
    memset(&msg, 0, sizeof(msg));
    if (!cnav_msg_decoder_add_symbol((cnav_msg_decoder_t*)h, symbol, &msg, &delay)) return 0;
    out5[0] = delay;
    out5[1] = msg.tow;
    out5[2] = msg.msg_id;
    out5[3] = msg.prn;
    out5[4] = msg.alert ? 1u : 0u;
    memcpy(raw64, msg.raw_msg, 64);
    return 1;
}

/* The scalar members of both parts, ten each: n_symbols, n_decoded, preamble_seen, invert, message_lock, crc_ok,
 * n_crc_fail, init, decisions_index, and whether old_metrics points at metrics2. */
void ref_cnav_scalars(void* h, int32_t* out20)
{
    cnav_msg_decoder_t* d = (cnav_msg_decoder_t*)h;
    const cnav_v27_part_t* parts[2] = {&d->part1, &d->part2};
    for (int k = 0; k < 2; k++) {
        const cnav_v27_part_t* p = parts[k];
        int32_t* o = out20 + 10 * k;
        o[0] = (int32_t)p->n_symbols;
        o[1] = (int32_t)p->n_decoded;
        o[2] = p->preamble_seen;
        o[3] = p->invert;
        o[4] = p->message_lock;
        o[5] = p->crc_ok;
        o[6] = (int32_t)p->n_crc_fail;
        o[7] = p->init;
        o[8] = (int32_t)p->dec.decisions_index;
        o[9] = p->dec.old_metrics == p->dec.metrics2;
    }
}

/* The arrays of one part: metrics1, metrics2 (64 each), the decisions (64 x 2 words), the symbol and decode buffers. */
void ref_cnav_arrays(void* h, int32_t part, uint32_t* metrics1, uint32_t* metrics2, uint32_t* decisions, uint8_t* symbols, uint8_t* decoded)
{
    cnav_msg_decoder_t* d = (cnav_msg_decoder_t*)h;
    const cnav_v27_part_t* p = part ? &d->part2 : &d->part1;
    memcpy(metrics1, p->dec.metrics1, sizeof(p->dec.metrics1));
    memcpy(metrics2, p->dec.metrics2, sizeof(p->dec.metrics2));
    for (int i = 0; i < 64; i++) {
        decisions[2 * i] = p->decisions[i].w[0];
        decisions[2 * i + 1] = p->decisions[i].w[1];
    }
    memcpy(symbols, p->symbols, sizeof(p->symbols));
    memcpy(decoded, p->decoded, sizeof(p->decoded));
}
