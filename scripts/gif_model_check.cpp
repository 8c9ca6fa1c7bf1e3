// gif_model_check.cpp — the GIF host model (gif_parse.hpp, gif_lzw.hpp: the text the kernels compile,
// the 64 lanes as a loop) as a stand-alone program, for runs under the host sanitizers:
//
//   hipcc --cuda-host-only -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o gif_model_check scripts/gif_model_check.cpp
//   ./gif_model_check file.gif ...
//
// Every buffer has exactly the size the device's regions have (align16(scan_len + 64) for the joined
// stream, w h + 64 for the indices, 3 w h for the pixels), so a read or write past one is reported.
// Prints per file: form (0 no GIF or a zero side, 1 Pillow's, 2 the device's), status, width, height and the
// FNV-1a hash of the RGB bytes (0 unless status is 0), which a caller compares with Pillow's pixels.
#include <stdio.h>

#include <vector>

#include "../dataloader_amd/csrc/gif_lzw.hpp"

int main(int argc, char** argv) {
  using namespace dino;
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) return 2;
    std::vector<uint8_t> file;
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + n);
    fclose(f);
    std::vector<uint8_t> exact(file);  // (capacity == size: the sanitizer sees the file's end)
    exact.shrink_to_fit();
    ImgDesc d{};
    d.status = DINO_IMG_CORRUPT;
    int form = 0, st = DINO_IMG_CORRUPT;
    unsigned long long h = 0;
    if (gif_signature(exact.data(), (int64_t)exact.size())) {  // (a zero side is corrupt: form 0, as dino_probe_gif says)
      const int hs = parse_gif_head(exact.data(), (int64_t)exact.size(), 65535, &d);
      form = hs == DINO_IMG_OK ? 2 : hs == DINO_IMG_CORRUPT ? 0 : 1;
    }
    if (form == 2) {
      const int64_t npx = (int64_t)d.width * d.height;
      std::vector<uint32_t> ent((size_t)(((int64_t)d.scan_len + 64 + 15) / 16 * 4));
      std::vector<uint8_t> plane((size_t)npx + 64), pal(kGifPalBytes), rgb((size_t)npx * 3);
      st = gif_decode_host(exact.data(), (int64_t)exact.size(), d, (uint8_t*)ent.data(), plane.data(), pal.data(), rgb.data());
      if (st == DINO_IMG_OK) {
        h = 1469598103934665603ull;
        for (uint8_t v : rgb) h = (h ^ v) * 1099511628211ull;
      }
    }
    printf("%s %d %d %d %d %llu\n", argv[a], form, st, form == 2 ? d.width : 0, form == 2 ? d.height : 0, h);
  }
  return 0;
}
