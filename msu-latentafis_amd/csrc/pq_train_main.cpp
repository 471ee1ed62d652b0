// pq_train — trains a PQ codebook over the texture descriptors of a directory of templates, on an MI355X through the C ABI: the command-line form of the
// reference's training (extraction/descriptor_PQ.py:41-77), beside pq_encode, which mirrors the same file's encoder.
//
//   pq_train --input_dir <dir>/ --output <codebook.dat> [--iters 20] [--seed 0] [--stride 2] [--min_points 100] [-d <device>]
//
// As in the reference: the directory argument is a string-prefix (it must end with '/'); texture template 0 of every file only (:49-51); a template with fewer than
// min_points texture points is skipped (:53-54); every stride-th point is taken, from the first (:58); 256 of the points initialise every sub-quantizer
// (minit='points', :73 — here afis_pq_train_init_points from --seed, reproducible) and 20 steps run unless --iters says otherwise (:70).
// Deliberate differences: inputs are in the matcher's own latent .dat layout (fp32 texture descriptors), the layout afis_encode_rolled_dat and pq_encode take; the
// files are taken in the order of their names; the reference's hard-coded file range 259 .. 1000 (:47) and its dead shuffle (:55-56: the permuted index array is
// never used) are not reproduced; the step is afis_pq_train's order-independent one and stops early at a fixed point.
// Prints one line per step (the labels that changed) and a summary (points, steps run, empty clusters).  Exit codes as pq_encode: 0, or 2 for a file, codebook or
// device failure.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/afis_matcher.h"
#include "pq_train_plan.h"
#include "template_io.h"

namespace fs = std::filesystem;
using namespace afis;

static std::string arg_of(int argc, char** argv, const char* name, const char* otherwise = "")
{
    for (int i = 1; i + 1 < argc; ++i) if (!strcmp(argv[i], name)) return argv[i + 1];
    return otherwise;
}

static std::vector<fs::path> glob_dat(const std::string& prefix)      // glob.glob(input_dir + '*.dat')
{
    std::vector<fs::path> out;
    const fs::path dir = fs::path(prefix).parent_path();
    const std::string stem_prefix = fs::path(prefix).filename().string();
    std::error_code ec;
    for (const auto& e : fs::directory_iterator(dir.empty() ? fs::path(".") : dir, ec)) {
        const std::string name = e.path().filename().string();
        if (e.is_regular_file() && e.path().extension() == ".dat" && name.compare(0, stem_prefix.size(), stem_prefix) == 0) out.push_back(e.path());
    }
    return out;
}

int main(int argc, char** argv)
{
    const std::string input_dir = arg_of(argc, argv, "--input_dir"), output = arg_of(argc, argv, "--output");
    if (input_dir.empty() || output.empty()) { std::cout << "Missing args." << std::endl; return 0; }
    const int iters = atoi(arg_of(argc, argv, "--iters", "20").c_str()), device = atoi(arg_of(argc, argv, "-d", "0").c_str());
    const uint64_t seed = strtoull(arg_of(argc, argv, "--seed", "0").c_str(), nullptr, 10);
    const int64_t stride = atoll(arg_of(argc, argv, "--stride", "2").c_str()), min_points = atoll(arg_of(argc, argv, "--min_points", "100").c_str());

    std::vector<fs::path> files = glob_dat(input_dir);
    std::sort(files.begin(), files.end(), [](const fs::path& a, const fs::path& b) { return a.filename().string() < b.filename().string(); });
    std::vector<float> des;
    std::vector<uint8_t> b;
    std::vector<int64_t> take;
    size_t used = 0;
    for (const fs::path& f : files) {
        if (!read_file(f.string(), b)) { std::cerr << "pq_train: cannot read " << f << std::endl; return 2; }
        HostTemplate t;
        if (parse_latent_dat(b.data(), b.size(), t) < 0 || t.tex.empty()) continue;            // :49-50
        const HostTexture& x = t.tex[0];
        if (x.des_len != 96 || x.des.size() != (size_t)x.n() * 96) { std::cerr << "pq_train: " << f << ": texture descriptors must be 96-d fp32" << std::endl; return 2; }
        take.clear();
        if (train_take_points(x.n(), min_points, stride, take) == 0) continue;
        for (int64_t i : take) des.insert(des.end(), x.des.begin() + i * 96, x.des.begin() + (i + 1) * 96);
        ++used;
    }
    const int64_t n = (int64_t)(des.size() / 96);
    std::vector<float> init(16 * 256 * 6), cw(16 * 256 * 6);
    std::vector<int64_t> counts(16 * 256), changed((size_t)std::max(iters, 1));
    int run = 0;
    if (afis_pq_train_init_points(des.data(), n, seed, init.data()) != AFIS_OK ||
        afis_pq_train(device, des.data(), n, init.data(), iters, cw.data(), counts.data(), changed.data(), &run) != AFIS_OK) {
        std::cerr << "pq_train: " << afis_last_error(nullptr) << " (" << n << " points of " << used << " templates)" << std::endl;
        return 2;
    }
    for (int t = 0; t < run; ++t) std::cout << "step " << t << ": changed " << changed[(size_t)t] << std::endl;
    size_t len = 0;
    afis_codebook_write(cw.data(), 16, 256, 6, nullptr, 0, &len);
    std::vector<uint8_t> out(len);
    if (afis_codebook_write(cw.data(), 16, 256, 6, out.data(), out.size(), &len) != AFIS_OK) { std::cerr << "pq_train: " << afis_last_error(nullptr) << std::endl; return 2; }
    std::ofstream of(output, std::ios::binary);
    of.write((const char*)out.data(), (std::streamsize)len);
    of.close();
    if (!of) { std::cerr << "pq_train: cannot write " << output << std::endl; return 2; }
    const long empty = (long)std::count(counts.begin(), counts.end(), (int64_t)0);
    std::cout << "pq_train: " << n << " points of " << used << " templates, " << run << " steps run, " << (run ? empty : 0) << " empty clusters -> " << output << std::endl;
    return 0;
}
