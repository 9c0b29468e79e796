// The Viterbi mirrors (include/gnsship_cpp.hpp Viterbi_Decoder_Hip, Galileo_Page_Decoder_Hip, galileo_*_vit_conf).
//   viterbi_mirror_test confs            prints the three page configurations (no GPU; tests/test_cpp_mirror_viterbi.py
//                                        compares them with the page sizes)
//   viterbi_mirror_test run FILE N       on the GPU: FILE holds N I/NAV frames of 240 float32 symbols.
//                                        One Viterbi_Decoder_Hip(7, 2, 114, {121, 91}) decodes them in order, with a
//                                        reset() ahead of the third: per frame a line "decode <f> <bits>" and a line
//                                        "section <f> <64 hex words>".  Then one Galileo_Page_Decoder_Hip takes the same
//                                        N frames as received pages of channels N-1 .. 0, the odd ones negated: a line
//                                        "frames <f> <bits>" each.  The Python test holds the expected values.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gnsship_cpp.hpp"

static void print_conf(const char* name, const gnsship_vit_conf& c)
{
    std::printf("%s constraint_length %d rate_n %d g0 %d g1 %d data_length %d interleaver_rows %d interleaver_cols %d invert_g2 %d mode %d\n", name,
        c.constraint_length, c.rate_n, c.g[0], c.g[1], c.data_length, c.interleaver_rows, c.interleaver_cols, c.invert_g2, c.mode);
}

static std::string bit_string(const uint8_t* b, size_t n)
{
    std::string s(n, '0');
    for (size_t i = 0; i < n; i++) s[i] = b[i] ? '1' : '0';
    return s;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "confs") == 0) {
        print_conf("inav", gnsship::galileo_inav_vit_conf());
        print_conf("fnav", gnsship::galileo_fnav_vit_conf());
        print_conf("cnav", gnsship::galileo_cnav_vit_conf(GNSSHIP_VIT_MODE_FULL));
        return 0;
    }
    if (argc != 4 || std::strcmp(argv[1], "run") != 0) {
        std::fprintf(stderr, "usage: viterbi_mirror_test confs | run FILE N\n");
        return 2;
    }
    const int n = std::atoi(argv[3]);
    const int LL = 114, frame = 240;
    if (n < 2 || n > 64) return 2;
    std::vector<float> sym(static_cast<size_t>(n) * frame);
    std::FILE* fp = std::fopen(argv[2], "rb");
    if (!fp || std::fread(sym.data(), sizeof(float), sym.size(), fp) != sym.size()) {
        std::fprintf(stderr, "cannot read %zu floats from %s\n", sym.size(), argv[2]);
        return 2;
    }
    std::fclose(fp);
    try {
        gnsship::Viterbi_Decoder_Hip dec(7, 2, LL, {121, 91});
        std::vector<int32_t> out(LL);
        for (int f = 0; f < n; f++) {
            if (f == 2) dec.reset();
            const std::vector<float> in(sym.begin() + static_cast<size_t>(f) * frame, sym.begin() + static_cast<size_t>(f + 1) * frame);
            dec.decode(out, in);
            std::vector<uint8_t> b(out.begin(), out.end());
            std::printf("decode %d %s\nsection %d", f, bit_string(b.data(), b.size()).c_str(), f);
            for (float v : dec.section()) {
                uint32_t w;
                std::memcpy(&w, &v, sizeof(w));
                std::printf(" %08x", w);
            }
            std::printf("\n");
        }
        gnsship::Galileo_Page_Decoder_Hip pages(gnsship::galileo_inav_vit_conf(), n);
        std::vector<int32_t> channels(static_cast<size_t>(n));
        std::vector<uint8_t> negate(static_cast<size_t>(n)), bits;
        for (int f = 0; f < n; f++) {
            channels[static_cast<size_t>(f)] = n - 1 - f;
            negate[static_cast<size_t>(f)] = static_cast<uint8_t>(f & 1);
        }
        if (pages.frame_symbols() != frame || pages.data_length() != LL || !pages.decode_frames(sym, channels, negate, bits)) {
            std::printf("decode_frames failed: %s\n", pages.last_error().c_str());
            return 1;
        }
        for (int f = 0; f < n; f++) std::printf("frames %d %s\n", f, bit_string(bits.data() + static_cast<size_t>(f) * LL, LL).c_str());
        // a channel twice in one call is refused in reference mode
        channels[0] = channels[1];
        std::printf("duplicate %s\n", pages.decode_frames(sym, channels, negate, bits) ? "accepted" : "refused");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("viterbi_mirror_test done\n");
    return 0;
}
