// tests/asan/fake_hip.h -- what the launcher stand-ins (sim_kernels.cpp) and the scenarios (host_sim.cpp) ask of the
// stand-in runtime (fake_hip.cpp) beyond the 27 HIP functions.  Test infrastructure only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fake {
// A launcher stand-in begins with op_begin: one operation on stream s (the host's clock goes into the stream, the
// stream's own component ticks).  The accesses that follow, up to the next operation, belong to it.
void op_begin(hipStream_t s, const char *name);
// [p, p + bytes) must lie wholly inside one live device block (bytes == 0: p inside or at the end of one).  Counts a
// violation and hands back false otherwise; `what` names the argument in the message.
bool in_block(const void *p, uint64_t bytes, const char *what);
// in_block, and the range noted as read or written by the current operation (the happens-before check)
bool dev_read(const void *p, uint64_t bytes, const char *what);
bool dev_write(const void *p, uint64_t bytes, const char *what);
// the whole block that holds p, for an argument whose extent the launcher cannot know
bool dev_read_block(const void *p, const char *what);
bool dev_write_block(const void *p, const char *what);
// a kernel's read of page-locked host memory (launch_copy_words): [p, p + bytes) must lie inside one page-locked range
bool pinned_read(const void *p, uint64_t bytes, const char *what);
// p is the base of a live device block of `bytes` bytes none of whose accesses is still unjoined into the host: what
// the library's pool promises of a block on its free list ("no kernel still uses the block")
bool quiescent(const void *p, uint64_t bytes, const char *what);
// the bytes left in p's block from p on (0: p is in no live block)
uint64_t room(const void *p);
// a violation of the caller's own finding, counted like the runtime's
void violation(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
// The host is told that [p, p + bytes) holds a result (an API call handed it back): a device-to-host Async copy into
// pageable memory that overlaps it and is not joined into the host is a violation.
void host_consumes(const void *p, uint64_t bytes, const char *what);
// after the last context is gone: no device block, page-locked range, stream or event may remain.  Prints the counts
// ("fake_hip: ... violations=N") and hands back the number of violations, leftovers included.
uint64_t finish(const char *scenario);
uint64_t violations();
// counts of what ran, for the log line
extern uint64_t n_launches;
}  // namespace fake
