// Stand-alone check of the fused decoder's threading (csrc/beam.cpp: amdspeech_ctc_beam_search_host_fused): the lockstep round pool
// under a sanitizer, with a C stub callback, no GPU and no Python.  Host code only:
//
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=thread -fsanitize=thread -x hip \
//           rnn-speech_amd/csrc/beam.cpp tools/beam_fused_tsan.cpp -o tools/beam_fused_tsan && tools/beam_fused_tsan
//
// (or -fsanitize=address).  Decodes one mini-batch of ragged lengths on 1, 2, 4 and 7 threads -- the same answer and at most T + 1
// callbacks each time -- and once with a callback that fails at its fifth call.  Exit status 0 and no sanitizer report: clean.
#include <cstdio>
#include <cstdarg>
#include <cstdlib>
#include <vector>
#include <cmath>
#include "../include/amdspeech.h"
namespace amdspeech {
void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
int runtime_switch(const char*, int d) { return d; }
}
static int calls = 0, fail_at = -1;
static int step(void* user, int n, const int* parent, const int* token, const int* dest, float* logq) {
    const int C = *static_cast<int*>(user);
    ++calls;
    if (calls == fail_at) return 7;
    for (int r = 0; r < n; ++r) {
        unsigned h = 2166136261u ^ (unsigned)parent[r] * 16777619u ^ (unsigned)token[r] * 40503u ^ (unsigned)dest[r];
        float z[64], s = 0;
        for (int c = 0; c < C; ++c) { h = h * 1664525u + 1013904223u; z[c] = (float)(h >> 8) / 16777216.0f; s += std::exp(z[c]); }
        for (int c = 0; c < C; ++c) logq[r * C + c] = z[c] - std::log(s);
    }
    return 0;
}
int main() {
    int T = 120, B = 7, C = 9, width = 12;
    std::vector<float> lg((size_t)T * B * C);
    unsigned h = 1;
    for (auto& v : lg) { h = h * 1664525u + 1013904223u; v = 3.0f * ((float)(h >> 8) / 16777216.0f - 0.5f); }
    std::vector<int> len = {120, 60, 0, 119, 1, 77, 120};
    std::vector<int> ids((size_t)B * 4 * T), out_len(B * 4), nf(B);
    std::vector<float> lp(B * 4);
    for (int threads : {1, 2, 4, 7}) {
        calls = 0; fail_at = -1;
        int rc = amdspeech_ctc_beam_search_host_fused(lg.data(), len.data(), T, B, C, width, 1, 4, 0.6f, 0.1f, step, &C, ids.data(), out_len.data(), lp.data(), nf.data(), threads);
        printf("threads %d rc %d calls %d best0 len %d score %f\n", threads, rc, calls, out_len[0], lp[0]);
        if (rc != 0 || calls > T + 1) return 1;
    }
    calls = 0; fail_at = 5;
    int rc = amdspeech_ctc_beam_search_host_fused(lg.data(), len.data(), T, B, C, width, 1, 0, 0.6f, 0.1f, step, &C, ids.data(), out_len.data(), lp.data(), nullptr, 4);
    printf("failing callback: rc %d calls %d\n", rc, calls);
    return (rc == 7 && calls == 5) ? 0 : 1;
}
