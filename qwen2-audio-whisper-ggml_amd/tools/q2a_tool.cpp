// q2a_tool — model-file tooling CLI ("the build's own loader and k-quant/Q8_0 quantizer
// for the unchanged ggml file"; the reference ships no quantize executable).
//
//   q2a_tool gen-model OUT {tiny|full|L,D,H,M} {f32|f16} [seed] [threads]
//   q2a_tool quantize IN OUT {q4_k|q5_k|q6_k|q8_0|q4_0} [threads]
//   q2a_tool synth-clip OUT.f32 N_SAMPLES CLIP_INDEX
//   q2a_tool gen-projector OUT D_IN D_OUT {f32|f16} [seed]   (Qwen2-Audio multi-modal projector, q2a_format.cpp)
//   q2a_tool mel MODEL WAV OUT   (normalised log-mel of WAV, raw f32 [n_mels][n_len]: the input of q2a_main -mel.
//                                 The one command that needs the GPU: it loads lib/libq2a.so at run time)
#include "../csrc/q2a_format.h"
#include "q2a_encoder.h"
#include "q2a_whisper.h"

#include <dlfcn.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int usage() {
    fprintf(stderr,
            "usage:\n  q2a_tool gen-model OUT {tiny|full|L,D,H,M} {f32|f16} [seed] [threads]\n"
            "  q2a_tool quantize IN OUT {q4_k|q5_k|q6_k|q8_0|q4_0} [threads]\n"
            "  q2a_tool synth-clip OUT.f32 N_SAMPLES CLIP_INDEX\n"
            "  q2a_tool gen-projector OUT D_IN D_OUT {f32|f16} [seed]\n"
            "  q2a_tool mel MODEL WAV OUT\n");
    return 1;
}

// log-mel of a WAV file through q2a_pcm_to_mel of lib/libq2a.so (beside this executable's directory), so that every
// other command keeps running on a machine without a GPU runtime
static int write_mel(const char * model, const char * wav, const char * out) {
    char exe[4096];
    const ssize_t n = readlink("/proc/self/exe", exe, sizeof(exe) - 1);
    if (n <= 0) return 2;
    exe[n] = 0;
    std::string dir(exe);
    dir.erase(dir.rfind('/'));
    void * lib = dlopen((dir + "/../lib/libq2a.so").c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!lib) { fprintf(stderr, "q2a_tool mel: %s\n", dlerror()); return 2; }
    const auto f_open = (decltype(&q2a_open)) dlsym(lib, "q2a_open");
    const auto f_close = (decltype(&q2a_close)) dlsym(lib, "q2a_close");
    const auto f_info = (decltype(&q2a_get_info)) dlsym(lib, "q2a_get_info");
    const auto f_mel = (decltype(&q2a_pcm_to_mel)) dlsym(lib, "q2a_pcm_to_mel");
    const auto f_err = (decltype(&q2a_last_error)) dlsym(lib, "q2a_last_error");
    const auto f_wav = (decltype(&q2a_read_wav)) dlsym(lib, "q2a_read_wav");
    const auto f_free = (decltype(&q2a_wav_free)) dlsym(lib, "q2a_wav_free");
    if (!f_open || !f_close || !f_info || !f_mel || !f_err || !f_wav || !f_free) return 2;
    float * pcm = nullptr;
    int64_t ns = 0;
    if (f_wav(wav, &pcm, &ns, nullptr, nullptr) != 0) { fprintf(stderr, "q2a_tool mel: failed to read WAV file '%s'\n", wav); return 2; }
    q2a_engine * e = f_open(model, 0);
    if (!e) { fprintf(stderr, "q2a_tool mel: %s\n", f_err()); f_free(pcm); return 3; }
    q2a_info info;
    f_info(e, &info);
    std::vector<float> mel((size_t) info.n_mels * (size_t) ((ns + 480000) / 160));
    int n_len = 0;
    const int rc = f_mel(e, pcm, (int) ns, mel.data(), (int64_t) mel.size(), &n_len);
    if (rc != Q2A_OK) fprintf(stderr, "q2a_tool mel: %s\n", f_err());
    f_close(e);
    f_free(pcm);
    if (rc != Q2A_OK) return 3;
    FILE * f = fopen(out, "wb");
    if (!f) return 2;
    const bool ok = fwrite(mel.data(), 4, (size_t) info.n_mels * n_len, f) == (size_t) info.n_mels * n_len;
    return fclose(f) == 0 && ok ? 0 : 2;
}

int main(int argc, char ** argv) {
    if (argc < 2) return usage();
    const std::string cmd = argv[1];
    if (cmd == "gen-model" && argc >= 5) {
        q2a_hparams hp;
        memset(&hp, 0, sizeof(hp));
        hp.n_vocab = 51866; hp.n_audio_ctx = 1500; hp.n_text_ctx = 448; hp.n_text_layer = 0; hp.n_mels = 128;
        const std::string cfg = argv[3];
        if (cfg == "tiny") { hp.n_audio_layer = 2; hp.n_audio_state = 256; hp.n_audio_head = 4; }
        else if (cfg == "full") { hp.n_audio_layer = 32; hp.n_audio_state = 1280; hp.n_audio_head = 20; }
        else if (sscanf(cfg.c_str(), "%d,%d,%d,%d", &hp.n_audio_layer, &hp.n_audio_state, &hp.n_audio_head, &hp.n_mels) != 4) return usage();
        hp.n_text_state = hp.n_audio_state;
        hp.n_text_head = hp.n_audio_head;
        hp.ftype = std::string(argv[4]) == "f32" ? 0 : 1;
        const uint64_t seed = argc > 5 ? strtoull(argv[5], nullptr, 0) : 0x51A2;
        const int nt = argc > 6 ? atoi(argv[6]) : 8;
        return q2a_write_synthetic_model(argv[2], &hp, seed, nt);
    }
    if (cmd == "quantize" && argc >= 5) {
        const std::string t = argv[4];
        const int qt = t == "q4_k" ? Q2A_TYPE_Q4_K : t == "q5_k" ? Q2A_TYPE_Q5_K : t == "q6_k" ? Q2A_TYPE_Q6_K : t == "q8_0" ? Q2A_TYPE_Q8_0 : t == "q4_0" ? Q2A_TYPE_Q4_0 : -1;
        if (qt < 0) return usage();
        return q2a_quantize_model(argv[2], argv[3], qt, argc > 5 ? atoi(argv[5]) : 8);
    }
    if (cmd == "synth-clip" && argc >= 5) {
        const long n = atol(argv[3]);
        std::vector<float> v((size_t) n);
        q2a_synth_clip(v.data(), n, atoi(argv[4]));
        FILE * f = fopen(argv[2], "wb");
        if (!f) return 2;
        fwrite(v.data(), 4, v.size(), f);
        fclose(f);
        return 0;
    }
    if (cmd == "gen-projector" && argc >= 6) {
        const uint64_t seed = argc > 6 ? strtoull(argv[6], nullptr, 0) : 0x51A2;
        return q2a_write_synthetic_projector(argv[2], atoi(argv[3]), atoi(argv[4]), std::string(argv[5]) == "f32" ? 0 : 1, seed);
    }
    if (cmd == "mel" && argc >= 5) return write_mel(argv[2], argv[3], argv[4]);
    return usage();
}
