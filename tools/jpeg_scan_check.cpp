// The host half of csrc/jpeg.hip over a list of files, as a stand-alone program: for a sanitizer build of the parser and the
// bit reader (damaged files are their daily bread), which must not be loaded into Python.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Iinclude face_vijnana_yolov3_amd/csrc/jpeg.hip face_vijnana_yolov3_amd/csrc/api.hip tools/jpeg_scan_check.cpp \
//         -o tools/jpeg_scan_check          (api.hip: the context's error and profile helpers the device half links against)
//   ./jpeg_scan_check FILE...          (or: ./jpeg_scan_check @LIST, one path per line)
//
// Every file is copied into a heap block of exactly its size and the coefficients into one of exactly total_coefs values, so a
// read or write one element outside either is reported.  The program uses no GPU.  Output: one summary line; exit status 0
// unless a file cannot be read.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "fv_hotpath.h"

int main(int argc, char** argv) {
    std::vector<std::string> paths;
    for (int i = 1; i < argc; ++i) {
        if (argv[i][0] == '@') {
            std::ifstream list(argv[i] + 1);
            for (std::string line; std::getline(list, line);)
                if (!line.empty()) paths.push_back(line);
        } else {
            paths.push_back(argv[i]);
        }
    }
    long refused_header = 0, refused_scan = 0, accepted = 0;
    for (const std::string& path : paths) {
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); return 2; }
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t* data = (uint8_t*)malloc(n > 0 ? n : 1);
        if (n > 0 && fread(data, 1, n, f) != (size_t)n) { fprintf(stderr, "cannot read %s\n", path.c_str()); return 2; }
        fclose(f);
        fv_jpeg_info info;
        if (fv_jpeg_parse(data, (size_t)n, &info) != 0 || (int64_t)info.width * info.height > 178956970) {
            ++refused_header;
        } else {
            int16_t* coefs = (int16_t*)malloc((size_t)info.total_coefs * sizeof(int16_t) + 1);
            const int rc = fv_jpeg_entropy_decode(data, (size_t)n, coefs, info.total_coefs);
            if (rc == 0) {
                ++accepted;
            } else {
                ++refused_scan;
            }
            free(coefs);
        }
        free(data);
    }
    printf("%zu files: %ld refused by the header parser, %ld refused by the scan decoder, %ld accepted\n", paths.size(), refused_header,
           refused_scan, accepted);
    return 0;
}
