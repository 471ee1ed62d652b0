// match_selftest — CPU-only checks of the host pieces of `match` (no GPU, no HIP context): used by tests/test_oracle.py and
// tests/test_sharding.py.  Kept out of the product binary.
//   match_selftest -selftest-args <opt> <tokens...>          flag parsing (cli_util.h) — pinned against matching/argparser.h
//   match_selftest -selftest-config <file> -key <key>        afis.config reader — pinned against the reference's JSON library
//   match_selftest -selftest-shards <weights file> -world N  shard cut rule (rank_exchange.cpp) — equals host/sharding.py
//   match_selftest -selftest-exchange                        rendezvous: rank 0's 128 bytes reach every rank (RANK/WORLD_SIZE/MASTER_* env)
//   match_selftest -selftest-allgather                       AFIS_EXCHANGE=tcp all-gather + the agreement point, N local ranks
//   match_selftest -selftest-groups <rows file> -per N [-plain]   the launch-group rule (afis_device.h: launch_group_cuts / launch_group_latents): cut positions for the listed latent texture row counts
//   match_selftest -selftest-offsets <counts file>          the gallery's derived offset tables (afis_offsets.h: derived_offsets) for the listed (minutiae, texture point) counts per template
//   match_selftest -selftest-merge <file>                    the exchange's merge of per-rank rank lists (rank_exchange.cpp: merge_topk) on gathered idx / score words
//   match_selftest -selftest-classes                        the candidate kernel's shape-class rule (afis_device.h: rt_max_rows) as a table: nR  L1 L2 L4  stride1 stride2 stride4
//   match_selftest -selftest-scratch <file>                  the candidate kernel's grid (afis_device.h: minu_cands_grid) and the scratch prepared for a search (minu_scratch_bytes): per line "max_nR s3_tie_order max_nL...", one max_nL per launch group
//   match_selftest -selftest-pairs-grid <file>               the candidate kernel's grid for a chunk of a pair-list call (afis_device.h: minu_cands_pairs_grid): per line "max_nL max_nR s3_tie_order n_cus lds_bytes_per_wg scratch_bytes_held n_pairs"
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <vector>

#include "afis_device.h"
#include "afis_offsets.h"
#include "cli_util.h"
#include "rank_exchange.h"

using namespace afis;

int main(int argc, char** argv)
{
    ArgParser args(argc, argv);
    if (args.cmdOptionExists("-selftest-classes")) {                            // host-side class rule of k_minu_cands_rt (no GPU): tests/test_host.py checks its invariants
        std::cout << rt_class_simi_floats(1) << " " << rt_class_simi_floats(2) << " " << rt_class_simi_floats(4) << " " << rt_class_keys_per_thread(1) << " " << rt_class_keys_per_thread(2) << " "
                  << rt_class_keys_per_thread(4) << " " << rt_class_max_rolled(4) << " " << rt_class_max_latent(4) << std::endl;
        for (int nR = 0; nR <= 2000; ++nR)
            std::cout << nR << " " << rt_max_rows(1, nR) << " " << rt_max_rows(2, nR) << " " << rt_max_rows(4, nR) << " " << rt_row_stride(1, nR) << " " << rt_row_stride(2, nR) << " " << rt_row_stride(4, nR) << std::endl;
        return 0;
    }
    if (args.cmdOptionExists("-selftest-scratch")) {                            // the candidate kernel's grid and the scratch prepared for a search's launch groups (no GPU): one group set per line
        std::ifstream f(args.getCmdOption("-selftest-scratch"));
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream in(line);
            int max_nR = 0, tie = 0, v; std::vector<int> nL;
            if (!(in >> max_nR >> tie)) continue;
            while (in >> v) nL.push_back(v);
            for (int n : nL) { const MinuGrid g = minu_cands_grid(n, max_nR, tie); std::cout << "grid " << n << " " << max_nR << " " << tie << " " << g.wg_floats << " " << g.n_wg << " " << g.bytes() << std::endl; }
            std::cout << "prepared " << minu_scratch_bytes(nL.data(), nL.size(), max_nR, tie) << std::endl;
        }
        return 0;
    }
    if (args.cmdOptionExists("-selftest-pairs-grid")) {                         // the candidate kernel's grid for a chunk of a pair-list call (no GPU): one case per line
        std::ifstream f(args.getCmdOption("-selftest-pairs-grid"));
        long long nL, nR, tie, cus, lds, held, pairs;
        while (f >> nL >> nR >> tie >> cus >> lds >> held >> pairs) {
            const MinuGrid g = minu_cands_pairs_grid((int)nL, (int)nR, (int)tie, (int)cus, (size_t)lds, (size_t)held, (size_t)pairs);
            std::cout << "pairs_grid " << nL << " " << nR << " " << tie << " " << cus << " " << lds << " " << held << " " << pairs << " " << g.wg_floats << " " << g.n_wg << " " << g.bytes() << std::endl;
        }
        return 0;
    }
    if (args.cmdOptionExists("-selftest-offsets")) {                          // the shard's derived tables (no GPU): one "minutiae texture-points" pair per line
        std::ifstream f(args.getCmdOption("-selftest-offsets"));
        std::vector<int32_t> mo{0}, to{0}, toff, qb, tb; long long a, b;
        while (f >> a >> b) { mo.push_back((int32_t)(mo.back() + a)); to.push_back((int32_t)(to.back() + b)); }
        int64_t nq = 0, nt = 0; int max_nR = 0;
        derived_offsets(mo, to, toff, qb, tb, nq, nt, max_nR);
        const size_t G = mo.size() - 1;
        std::cout << G << " " << mo[G] << " " << to[G] << " " << toff[G] << " " << nq << " " << nt << " " << max_nR << std::endl;
        // every table in full would be 3 x 10^6 lines: weighted sums modulo 2^64 over all entries, then every 997th entry and the last
        unsigned long long h[3] = {0, 0, 0};
        for (size_t t = 0; t <= G; ++t) { const unsigned long long w = 2 * (unsigned long long)t + 1; h[0] += w * (unsigned long long)toff[t]; h[1] += w * (unsigned long long)qb[t]; h[2] += w * (unsigned long long)tb[t]; }
        std::cout << h[0] << " " << h[1] << " " << h[2] << std::endl;
        for (size_t t = 0;; t = std::min(t + 997, G)) { std::cout << t << " " << toff[t] << " " << qb[t] << " " << tb[t] << std::endl; if (t == G) break; }
        return 0;
    }
    if (args.cmdOptionExists("-selftest-groups")) {                             // the launch-group rule (no GPU): rows per latent (one int per line), latents per launch at most
        std::ifstream f(args.getCmdOption("-selftest-groups"));
        std::vector<long long> pre{0}; long long v;
        while (f >> v) pre.push_back(pre.back() + v);
        const int n = (int)pre.size() - 1, per = atoi(args.getCmdOption("-per").c_str());
        std::vector<int> cuts((size_t)(n > 0 ? n : 1)); int m = 0;
        launch_group_cuts(pre.data(), n, per, !args.cmdOptionExists("-plain"), cuts.data(), &m);
        for (int i = 0; i < m; ++i) std::cout << cuts[(size_t)i] << (i + 1 < m ? " " : "");
        std::cout << std::endl;
        for (long long G : {1ll, 12500ll, 39000ll, 40000ll, 50000ll, 100000ll, 250000ll, 500000ll, 1000000ll}) std::cout << G << ":" << launch_group_latents(G) << " ";
        std::cout << std::endl;
        return 0;
    }
    if (args.cmdOptionExists("-selftest-exchange")) {                           // rendezvous only (no GPU): rank 0's 128 bytes reach every rank
        RankWorld w; world_from_env(w);
        unsigned char id[128];
        for (int i = 0; i < 128; ++i) id[i] = w.rank == 0 ? (unsigned char)(i * 7 + 3) : 0;
        std::string err;
        if (!tcp_broadcast(w, id, sizeof(id), err)) { std::cerr << "match: " << err << std::endl; return 2; }
        unsigned sum = 0; for (int i = 0; i < 128; ++i) sum = sum * 31 + id[i];
        std::cout << "rank " << w.rank << " of " << w.world << " id " << sum << std::endl;
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "-selftest-args")) {                      // token rules (no GPU): match -selftest-args <opt> <tokens...>
        ArgParser rest(argc - 2, argv + 2);                                     // argv[2] plays the program name, as argv[0] would
        std::cout << "exists=" << (rest.cmdOptionExists(argv[2]) ? 1 : 0) << " value=" << rest.getCmdOption(argv[2]) << std::endl;
        return 0;
    }
    if (args.cmdOptionExists("-selftest-config")) {                             // config reader (no GPU): match -selftest-config <file> -key <key>
        const auto kv = read_flat_json(args.getCmdOption("-selftest-config"));
        const auto it = kv.find(args.getCmdOption("-key"));
        std::cout << "found=" << (it != kv.end() ? 1 : 0) << " value=" << (it != kv.end() ? it->second : std::string()) << std::endl;
        return 0;
    }
    if (args.cmdOptionExists("-selftest-shards")) {                             // shard cut rule (no GPU): weights file (one int per line), world
        std::ifstream f(args.getCmdOption("-selftest-shards"));
        std::vector<int32_t> wts; int v;
        while (f >> v) wts.push_back(v);
        const int world = atoi(args.getCmdOption("-world").c_str());
        for (const auto& b : shard_bounds((int64_t)wts.size(), wts, world)) std::cout << b.first << " " << b.second << std::endl;
        std::vector<int32_t> none;
        for (const auto& b : shard_bounds((int64_t)wts.size(), none, world)) std::cout << b.first << " " << b.second << std::endl;
        return 0;
    }
    if (args.cmdOptionExists("-selftest-merge")) {                              // the exchange's merge (no GPU): "world k k_out", then world * k lines "idx score-word-in-hex"; prints k_out such lines
        std::ifstream f(args.getCmdOption("-selftest-merge"));
        int world = 0, k = 0, k_out = 0;
        if (!(f >> world >> k >> k_out) || world < 1 || k < 0 || k_out < 0) { std::cerr << "match_selftest: bad merge file" << std::endl; return 2; }
        std::vector<int64_t> idx((size_t)world * k), out_i; std::vector<float> sc((size_t)world * k), out_s;
        for (size_t i = 0; i < idx.size(); ++i) {
            long long v; std::string w;
            if (!(f >> v >> w)) { std::cerr << "match_selftest: short merge file" << std::endl; return 2; }
            const uint32_t bits = (uint32_t)strtoul(w.c_str(), nullptr, 16);
            idx[i] = v; memcpy(&sc[i], &bits, 4);
        }
        merge_topk(idx, sc, world, k, k_out, out_i, out_s);
        for (size_t r = 0; r < out_i.size(); ++r) { uint32_t bits; memcpy(&bits, &out_s[r], 4); std::cout << out_i[r] << " " << std::hex << bits << std::dec << std::endl; }
        return 0;
    }
    if (args.cmdOptionExists("-selftest-allgather")) {                         // tcp all-gather of rank-dependent blocks, then world_agree
        RankWorld w; world_from_env(w);
        std::string err;
        setenv("AFIS_EXCHANGE", "tcp", 1);
        if (!world_init(w, 0, err)) { std::cerr << err << std::endl; return 2; }
        const size_t n = 1000 + 17;
        std::vector<uint32_t> mine(n), all(n * (size_t)w.world);
        for (size_t i = 0; i < n; ++i) mine[i] = (uint32_t)(w.rank * 1000003u + i * 7u);
        for (int round = 0; round < 3; ++round) {
            if (!world_all_gather(w, mine.data(), all.data(), n * sizeof(uint32_t), err)) { std::cerr << err << std::endl; return 2; }
            for (int r = 0; r < w.world; ++r)
                for (size_t i = 0; i < n; ++i) if (all[(size_t)r * n + i] != (uint32_t)(r * 1000003u + i * 7u)) { std::cerr << "bad block" << std::endl; return 3; }
        }
        const int fail_rank = atoi(args.getCmdOption("-fail-rank").c_str());   // that rank reports code 7 (0: nobody fails)
        const int code = world_agree(w, (fail_rank > 0 && w.rank == fail_rank) ? 7 : 0, err);
        std::cout << "rank " << w.rank << " of " << w.world << " gathered ok, agree " << code << std::endl;
        world_finalize(w);
        return 0;
    }
    std::cerr << "match_selftest: no check named" << std::endl;
    return 2;
}
