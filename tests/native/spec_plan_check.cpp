// Replays whisperkit_amd/csrc/spec_plan.h on a model of the self-attention cache (tests/test_speculative_plan.py; g++ -O2 -Wall -Werror).
// The model: cell (slot, row) remembers which audio wrote it, for which position and with which input token.  The target is a fixed greedy sequence
// per audio - what it samples at a position whose history is the confirmed one - so a look-ahead position is kept exactly when the input it was fed is
// the token the target sampled before it (inside the prompt: always, the loop forces those - but for the decode loop's one exception: a prompt that ends
// in a timestamp has that token REPLACED by the timestamp the target predicted before it, `replaced`, and the look-ahead into that position, armed with
// the prompt's own token, is then not kept).  Queries on stdin, one answer line each:
//   sched K n_prompt limit eot replaced | g0 g1 ... | d0 d1 ...      the round schedule of one audio: "rounds positions accepted"
//   replay seed K n_audio max_batch iters                    random prompts (1 .. 100), sequences, proposals and acceptance patterns: "ok <positions checked>"
//   fits n_audio K max_batch                                 "<spec_fits> <last slot of the last audio>"
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "spec_plan.h"

using namespace wh::plan;

struct Cell { int audio = -1, position = -1, input = -1; };

struct Audio {
    int n_prompt = 1, limit = 1, eot = 0;
    bool replaced = false;      // the target replaces the prompt's last token (a timestamp) by its own prediction
    std::vector<int32_t> prompt, greedy, proposals;      // greedy[i]: the target's sample at position n_prompt - 1 + i
    int input(int p) const {                                     // the confirmed input of position p
        if (replaced && p == n_prompt - 1 && p > 0) return prompt[(size_t)p] + 1000;
        return p < n_prompt ? prompt[(size_t)p] : greedy[(size_t)(p - n_prompt)];
    }
};

// one audio's pass over the cache model; returns an error text or "".  check_cache = false: the schedule alone
static std::string run_audio(const Audio& A, int a, int K, int max_batch, std::vector<std::vector<Cell>>* cache, SpecCounters& c, long long* checked) {
    int p0 = 0;
    char buf[256];
    while (true) {
        if (A.limit < 1) return "";
        const int k = spec_lookahead(p0, K, A.n_prompt, A.limit, A.proposals.data(), (int)A.proposals.size(), A.eot);
        if (k < 0 || k > K || p0 + k >= A.limit) { snprintf(buf, sizeof(buf), "audio %d: look-ahead %d from %d (K %d, limit %d)", a, k, p0, K, A.limit); return buf; }
        // the round's inputs: the known one, then the prompt or the proposals
        std::vector<int> in((size_t)k + 1);
        in[0] = A.input(p0);
        for (int j = 1; j <= k; ++j) { const int p = p0 + j; in[(size_t)j] = p < A.n_prompt ? A.prompt[(size_t)p] : A.proposals[(size_t)(p - A.n_prompt)]; }
        if (cache) {
            // every position of the launch writes its row before any position reads (the QKV projection precedes the attention launch)
            for (int j = 0; j <= k; ++j) {
                const int p = p0 + j, slot = spec_slot(a, K, p);
                if (slot < spec_first_slot(a, K) || slot >= spec_first_slot(a + 1, K) || slot >= max_batch) { snprintf(buf, sizeof(buf), "audio %d: position %d runs in slot %d outside its range", a, p, slot); return buf; }
                for (int i = 0; i < j; ++i) if (spec_slot(a, K, p0 + i) == slot) { snprintf(buf, sizeof(buf), "audio %d: positions %d and %d of one round share slot %d", a, p0 + i, p, slot); return buf; }
                Cell& cell = (*cache)[(size_t)slot][(size_t)p];
                if (cell.audio >= 0 && cell.audio != a) { snprintf(buf, sizeof(buf), "audio %d overwrites a cell of audio %d", a, cell.audio); return buf; }
                cell = Cell{a, p, in[(size_t)j]};
            }
        }
        // how far the target agrees
        int j = 0;
        bool done = false;
        while (true) {
            const int p = p0 + j;
            if (in[(size_t)j] != A.input(p)) { snprintf(buf, sizeof(buf), "audio %d: position %d was kept on input %d, confirmed %d", a, p, in[(size_t)j], A.input(p)); return buf; }
            if (cache) {
                for (int q = 0; q <= p; ++q) {            // every row the position reads: last written by a run of that row's position with the confirmed input
                    const int slot = spec_slot(a, K, q);
                    const Cell& cell = (*cache)[(size_t)slot][(size_t)q];
                    if (cell.audio != a || cell.position != q || cell.input != A.input(q)) {
                        snprintf(buf, sizeof(buf), "audio %d: position %d reads row %d in slot %d: written by audio %d position %d input %d, confirmed input %d", a, p, q, slot,
                                 cell.audio, cell.position, cell.input, A.input(q));
                        return buf;
                    }
                }
                ++*checked;
            }
            int sample = -1;
            if (p >= A.n_prompt - 1) { sample = A.greedy[(size_t)(p - (A.n_prompt - 1))]; if (sample == A.eot) done = true; }
            if (p + 1 >= A.limit) done = true;
            if (done || j == k) break;
            if (p + 1 >= A.n_prompt ? in[(size_t)j + 1] != sample : in[(size_t)j + 1] != A.input(p + 1)) break;
            ++j;
        }
        c.round(k, j);
        if (done) return "";
        p0 += j + 1;
    }
}

static std::vector<int32_t> ints(const std::string& s) {
    std::istringstream is(s);
    std::vector<int32_t> v;
    long long x;
    while (is >> x) v.push_back((int32_t)x);
    return v;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        if (cmd == "sched") {
            std::string rest;
            std::getline(is, rest);
            std::vector<std::string> part;
            std::istringstream rs(rest);
            for (std::string p; std::getline(rs, p, '|');) part.push_back(p);
            while (part.size() < 3) part.push_back("");
            const std::vector<int32_t> h = ints(part[0]);
            Audio A;
            const int K = h[0];
            A.n_prompt = h[1]; A.limit = h[2]; A.eot = h[3]; A.replaced = h[4] != 0;
            A.prompt.assign((size_t)A.n_prompt, A.eot + 1);
            A.greedy = ints(part[1]); A.proposals = ints(part[2]);
            A.greedy.resize((size_t)A.limit + 2, A.eot);      // (never read beyond the sequence's end: the limit or the end token stops the walk first)
            SpecCounters c;
            const std::string e = run_audio(A, 0, K, K + 1, nullptr, c, nullptr);
            if (!e.empty()) printf("fail %s\n", e.c_str());
            else printf("%lld %lld %lld\n", c.rounds, c.positions_run, c.tokens_accepted);
        } else if (cmd == "replay") {
            unsigned seed; int K, n_audio, max_batch, iters;
            is >> seed >> K >> n_audio >> max_batch >> iters;
            std::mt19937 rng(seed);
            auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
            long long checked = 0;
            std::string err;
            if (!spec_fits(n_audio, K, max_batch)) err = "does not fit";
            for (int it = 0; it < iters && err.empty(); ++it) {
                std::vector<std::vector<Cell>> cache((size_t)max_batch, std::vector<Cell>(224));
                std::vector<Audio> au((size_t)n_audio);
                for (Audio& A : au) {
                    A.eot = 7;
                    A.n_prompt = rnd(1, 100);
                    A.replaced = rnd(0, 1) == 1;
                    A.limit = rnd(0, 3) ? rnd(A.n_prompt, 223) : rnd(1, 223);          // mostly beyond the prompt, sometimes inside it
                    A.prompt.resize((size_t)A.n_prompt);
                    for (auto& t : A.prompt) t = rnd(8, 40);
                    const int n = rnd(0, 223);                                       // samples before the end token (or the limit)
                    A.greedy.resize(224 + 2);
                    for (size_t i = 0; i < A.greedy.size(); ++i) A.greedy[i] = (int)i < n ? rnd(8, 40) : A.eot;
                    // proposals: the sequence itself with a random corruption pattern, a random length, sometimes an end token in the middle
                    const int pattern = rnd(0, 4), np = rnd(0, 4) ? rnd(0, 223) : 0;
                    A.proposals.resize((size_t)np);
                    for (int i = 0; i < np; ++i) {
                        int t = A.greedy[(size_t)i];
                        const bool wrong = pattern == 0 ? false : pattern == 1 ? true : pattern == 2 ? i % 3 == 2 : pattern == 3 ? i % 7 == 6 : rnd(0, 3) == 0;
                        if (wrong) t = t == 41 ? 42 : 41;
                        A.proposals[(size_t)i] = t;
                    }
                    if (np > 4 && rnd(0, 3) == 0) A.proposals[(size_t)rnd(0, np - 1)] = A.eot;
                }
                // the audios' rounds interleave in a real pass; their cells are disjoint, so the order does not matter to the model: checked by the owner test in run_audio
                SpecCounters c;
                for (int a = 0; a < n_audio && err.empty(); ++a) err = run_audio(au[(size_t)a], a, K, max_batch, &cache, c, &checked);
                for (int s = 0; s < max_batch && err.empty(); ++s)
                    for (const Cell& cell : cache[(size_t)s])
                        if (cell.audio >= 0 && (s < spec_first_slot(cell.audio, K) || s >= spec_first_slot(cell.audio + 1, K))) err = "a cell outside its audio's slot range";
            }
            if (!err.empty()) printf("fail %s\n", err.c_str());
            else printf("ok %lld\n", checked);
        } else if (cmd == "fits") {
            int n_audio, K, max_batch;
            is >> n_audio >> K >> max_batch;
            printf("%d %d\n", spec_fits(n_audio, K, max_batch) ? 1 : 0, spec_k_valid(K) && n_audio >= 1 ? spec_slot(n_audio - 1, K, K) : -1);
        } else {
            printf("unknown\n");
        }
        fflush(stdout);
    }
    return 0;
}
