// TEST INFRASTRUCTURE ONLY -- a second checker over the reference C++ engine, next to its own nnue_inference tool.
//
// The reference's tool always evaluates layer stack 0 and prints no feature ids.  This driver calls the same public entry
// points (nnue_engine.h is found on the include path oracle/Makefile sets; the engine's sources are compiled where they
// lie) with a layer stack index of the caller's choice, for several images and indices per process:
//
//   engine_driver [--bits] <model.nnue> <images.bin> <H> <W> <count> <k> [<k> ...]
//
// images.bin holds `count` buffers of 3*H*W float32 each, handed to the engine as they stand.  One line per (image, k):
//
//   <image> <k> | <logit>,<logit>,... | <density> | <id> <id> ...
//
// logits and density with ten fixed decimals (the tool's format; density = float(active ids) / float(total features), its
// expression), the ids as the engine returns them after that very call.  A call that returns no logits ends the run with
// status 2.  Ten decimals are exact for multiples of 1/64 but not for a quotient by 3.0 or 0.1: with the leading flag --bits
// every logit and the density are printed as the eight hex digits of their float32 bit pattern instead (the rest of the line,
// and the output without the flag, are unchanged).
#include <nnue_engine.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static void print_float(float v, bool bits) {
    if (!bits) {
        std::printf("%.10f", static_cast<double>(v));
        return;
    }
    std::uint32_t u;
    std::memcpy(&u, &v, sizeof u);
    std::printf("%08x", static_cast<unsigned>(u));
}

int main(int argc, char** argv) {
    const char* program = argv[0];
    const bool bits = argc > 1 && std::strcmp(argv[1], "--bits") == 0;
    if (bits) {
        ++argv;
        --argc;
    }
    if (argc < 7) {
        std::fprintf(stderr, "usage: %s [--bits] <model.nnue> <images.bin> <H> <W> <count> <k> [<k> ...]\n", program);
        return 1;
    }
    const int h = std::atoi(argv[3]), w = std::atoi(argv[4]), count = std::atoi(argv[5]);
    if (h <= 0 || w <= 0 || count <= 0) {
        std::fprintf(stderr, "H, W and count must be positive\n");
        return 1;
    }
    const size_t per_image = static_cast<size_t>(h) * static_cast<size_t>(w) * 3;
    std::vector<float> images(per_image * static_cast<size_t>(count));
    std::FILE* f = std::fopen(argv[2], "rb");
    if (f == nullptr || std::fread(images.data(), sizeof(float), images.size(), f) != images.size()) {
        std::fprintf(stderr, "%s: cannot read %d images of %zu floats\n", argv[2], count, per_image);
        return 1;
    }
    std::fclose(f);

    nnue::NNUEEvaluator engine;
    if (!engine.load_model(argv[1])) {
        std::fprintf(stderr, "%s: the engine refuses the model\n", argv[1]);
        return 1;
    }
    const int total = engine.get_total_features();
    for (int i = 0; i < count; ++i) {
        const float* image = images.data() + per_image * static_cast<size_t>(i);
        for (int a = 6; a < argc; ++a) {
            const int k = std::atoi(argv[a]);
            const std::vector<float> logits = engine.evaluate_logits(image, h, w, k);
            if (logits.empty()) {
                std::fprintf(stderr, "image %d, layer stack %d: the engine returned no logits\n", i, k);
                return 2;
            }
            std::vector<int> ids;
            engine.get_active_features(ids);
            const float density = total > 0 ? static_cast<float>(ids.size()) / total : 0.0f;
            std::printf("%d %d |", i, k);
            for (size_t c = 0; c < logits.size(); ++c) {
                std::printf("%s", c ? "," : " ");
                print_float(logits[c], bits);
            }
            std::printf(" | ");
            print_float(density, bits);
            std::printf(" |");
            for (int id : ids) std::printf(" %d", id);
            std::printf("\n");
        }
    }
    return 0;
}
