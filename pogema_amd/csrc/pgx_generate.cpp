// pgx_generate.cpp -- the host-side synthetic map generator of the C-ABI (pgx_generate, pgx_place_agents).
//
// Instance generator "GEN v2", host side.  Counter-based so that the device kernels (pgx_reset_random) draw the very same
// instances -- both take the hash and its keys from pgx_internal.h:
//   h = mix(seed, global env, epoch, attempt);  obstacle(c) <=> hash(h, 'OBST', c) >> 40 < thr;
//   candidates c_t = hash(h, 'PLAC', t) scaled to [0, cells); first visit of a component opens a pair,
//   the next visit closes it.  Normative statement: oracle/generator_oracle.py (test infrastructure).
#include "../../include/pogema_amd.h"

#include <algorithm>
#include <thread>
#include <vector>

#include "pgx_internal.h"

namespace {

using pgx::fail_msg;

struct GenScratch {
    std::vector<int32_t> label, stack, pending;
    std::vector<uint8_t> taken;
};

void label_min_index(const uint8_t* obst, int H, int Wd, GenScratch& g) {
    const int cells = H * Wd;
    g.label.assign(cells, -1);
    for (int s = 0; s < cells; ++s) {
        if (obst[s] || g.label[s] >= 0) continue;
        g.label[s] = s;  // row-major scan: the first cell reached is the component's smallest index
        g.stack.clear();
        g.stack.push_back(s);
        while (!g.stack.empty()) {
            const int c = g.stack.back();
            g.stack.pop_back();
            const int x = c / Wd, y = c - x * Wd;
            const int nb[4] = {x > 0 ? c - Wd : -1, x + 1 < H ? c + Wd : -1, y > 0 ? c - 1 : -1, y + 1 < Wd ? c + 1 : -1};
            for (int k = 0; k < 4; ++k) {
                const int n = nb[k];
                if (n >= 0 && !obst[n] && g.label[n] < 0) {
                    g.label[n] = s;
                    g.stack.push_back(n);
                }
            }
        }
    }
}

// one env, one attempt; returns true when `A` start/target pairs were placed
// (obst_out == nullptr: place on the given `obst_in` map instead of drawing one; labels then reused)
bool generate_one(int H, int Wd, int A, uint32_t thr, uint64_t h, const uint8_t* obst_in, uint8_t* obst_out,
                  bool relabel, int32_t* axy, int32_t* txy, GenScratch& g) {
    const int cells = H * Wd;
    if (obst_out)
        for (int c = 0; c < cells; ++c)
            obst_out[c] = (pgx::gen_sm64(h ^ (pgx::GEN_TAG_OBST | (uint64_t)c)) >> 40) < thr ? 1 : 0;
    const uint8_t* obst = obst_out ? obst_out : obst_in;
    if (relabel) label_min_index(obst, H, Wd, g);
    g.taken.assign(cells, 0);
    g.pending.assign(cells, -1);
    int placed = 0;
    const uint32_t budget = pgx::gen_candidate_budget((uint32_t)cells);
    for (uint32_t t = 0; t < budget && placed < A; ++t) {
        const uint32_t c = (uint32_t)(((pgx::gen_sm64(h ^ (pgx::GEN_TAG_PLACE | (uint64_t)t)) >> 32) * (uint64_t)cells) >> 32);
        if (obst[c] || g.taken[c]) continue;
        g.taken[c] = 1;
        int32_t& open = g.pending[g.label[c]];
        if (open < 0) {
            open = (int32_t)c;
        } else {
            axy[2 * placed] = open / Wd;
            axy[2 * placed + 1] = open % Wd;
            txy[2 * placed] = (int32_t)c / Wd;
            txy[2 * placed + 1] = (int32_t)c % Wd;
            open = -1;
            ++placed;
        }
    }
    return placed == A;
}

// Draws every env b of the batch on `nthreads` threads (<= 0: one per hardware thread): attempt(b, k, scratch) for
// k = 0, 1, ... until it succeeds or `max_retries` attempts are spent.  Returns an env that failed (the first one of
// the lowest thread that had a failure), or -1.
template <class Attempt>
int64_t generate_batch(int32_t batch, int32_t max_retries, int32_t nthreads, const Attempt& attempt) {
    unsigned nt = nthreads > 0 ? (unsigned)nthreads : std::max(1u, std::thread::hardware_concurrency());
    nt = (unsigned)std::min<int64_t>(nt, batch);
    std::vector<int64_t> failed(nt, -1);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t) {
        pool.emplace_back([&, t]() {
            GenScratch g;
            for (int64_t b = t; b < batch; b += nt) {
                bool ok = false;
                for (int k = 0; k < max_retries && !ok; ++k) ok = attempt(b, k, g);
                if (!ok && failed[t] < 0) failed[t] = b;
            }
        });
    }
    for (auto& th : pool) th.join();
    for (unsigned t = 0; t < nt; ++t)
        if (failed[t] >= 0) return failed[t];
    return -1;
}

}  // namespace

extern "C" {

int pgx_generate(int32_t batch, int32_t height, int32_t width, int32_t num_agents, float density, uint64_t seed0,
                 int64_t env_index_base, int32_t max_retries, int32_t nthreads, uint8_t* obstacles, int32_t* agent_xy,
                 int32_t* target_xy) {
    if (batch < 1 || height < 1 || width < 1 || num_agents < 1 || !obstacles || !agent_xy || !target_xy)
        return fail_msg(PGX_E_INVALID, "pgx_generate: bad argument");
    if (!(density >= 0.0f && density <= 1.0f)) return fail_msg(PGX_E_INVALID, "density %.3f outside [0, 1]", (double)density);
    if ((int64_t)2 * num_agents > (int64_t)height * width)
        return fail_msg(PGX_E_PLACEMENT, "%d agents need %d distinct cells, map has %d", num_agents, 2 * num_agents,
                        height * width);
    if (max_retries < 1) max_retries = 10;
    const uint32_t thr = pgx::gen_density_threshold(density);
    const size_t cells = (size_t)height * width;
    const int64_t failed = generate_batch(batch, max_retries, nthreads, [&](int64_t b, int attempt, GenScratch& g) {
        // env b of the call is global env (env_index_base + b) of stream `seed0`: shards and single-env calls draw the
        // same instances, and different seeds share none
        const uint64_t h = pgx::gen_instance_hash(seed0, (uint64_t)(env_index_base + b), 0, (uint32_t)attempt);
        return generate_one(height, width, num_agents, thr, h, nullptr, obstacles + b * cells, true,
                            agent_xy + (size_t)b * num_agents * 2, target_xy + (size_t)b * num_agents * 2, g);
    });
    if (failed >= 0)
        return fail_msg(PGX_E_PLACEMENT, "could not place %d agents in env %d after %d attempts (density %.2f, %dx%d)",
                        num_agents, (int)failed, max_retries, (double)density, height, width);
    return PGX_OK;
}

int pgx_place_agents(int32_t batch, int32_t height, int32_t width, int32_t num_agents, uint64_t seed0,
                     int64_t env_index_base, int32_t max_retries, int32_t nthreads, const uint8_t* obstacles,
                     int32_t shared_map, int32_t* agent_xy, int32_t* target_xy) {
    if (batch < 1 || height < 1 || width < 1 || num_agents < 1 || !obstacles || !agent_xy || !target_xy)
        return fail_msg(PGX_E_INVALID, "pgx_place_agents: bad argument");
    if (max_retries < 1) max_retries = 10;
    const size_t cells = (size_t)height * width;
    const int64_t failed = generate_batch(batch, max_retries, nthreads, [&](int64_t b, int attempt, GenScratch& g) {
        const uint8_t* m = obstacles + (shared_map ? 0 : b * cells);
        const uint64_t h = pgx::gen_instance_hash(seed0, (uint64_t)(env_index_base + b), 0, (uint32_t)attempt);
        return generate_one(height, width, num_agents, 0u, h, m, nullptr, attempt == 0 || !shared_map,
                            agent_xy + (size_t)b * num_agents * 2, target_xy + (size_t)b * num_agents * 2, g);
    });
    if (failed >= 0)
        return fail_msg(PGX_E_PLACEMENT, "could not place %d agents on the given map of env %d after %d attempts",
                        num_agents, (int)failed, max_retries);
    return PGX_OK;
}

}  // extern "C"
