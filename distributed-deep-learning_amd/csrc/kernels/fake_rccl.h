// A fake RCCL for one process on one card (fake_rccl.hip): the table behind rccl_api.h's override
// seam.  Test support only, reachable through the explicit bindings and nothing else.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace ddl {
namespace fake_rccl {

struct Buffer {
  float* base = nullptr;
  int64_t n = 0;
};

struct Config {
  int world = 1, rank = 0;
  Buffer params, grads;        // the rank's live buffers (the same length)
  std::vector<Buffer> shards;  // every unit's reduce-scatter receive buffer
  float* seen = nullptr;       // optional [total]: every reduction's send range, copied first
};

// What the peers hold.  kTable: peer_grads / params_next of set_step.  kPattern: the runner's
// self-test pattern, rank q holding (q + 1) * (i % 13 + 1) at element i of an unregistered buffer.
enum Peers { kTable = 0, kPattern = 1 };
enum Fault { kNone = 0, kRsNextChunk, kAgSkip, kReduceDropPeer, kBcastSkip };

struct Call {
  std::string op, buf, rbuf;  // buf / off: the send side; rbuf / roff: the receive side
  int64_t off = -1, roff = -1, count = 0;
  int root = -1;
  uint64_t stream = 0;
  int depth = 0;
};

void install(const Config& c);  // configure, clear both lists, put the table into the seam
void remove();                  // take it out again (refused while a communicator lives)
void set_step(const float* peer_grads, const float* params_next);  // [W, total] and [total]
void set_peers(int peers);
void set_fault(int fault);
void clear();
std::vector<Call> calls();
std::vector<std::string> violations();
int group_depth();
bool overridden();  // any table in the seam (rccl_api.h rccl_overridden)

}  // namespace fake_rccl
}  // namespace ddl
