/*
 * bpftime_amd runtime C ABI (libbpftime_amd.so): device-resident maps, the
 * prog / bpf_link records of the XDP attach surface, and device utilities.
 *
 * The map / prog / link entry points keep the names, argument meaning and
 * error conventions of the reference's shared-memory runtime
 * (runtime/include/bpftime_shm.hpp:220-400, implemented in
 * runtime/src/bpftime_shm.cpp:69-140 / bpftime_shm_internal.cpp), with the
 * map storage living in GPU HBM instead of a boost.interprocess segment.
 */
#ifndef BPFTIME_AMD_H
#define BPFTIME_AMD_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include "ebpf-vm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* runtime/include/bpftime_shm.hpp:27-46 (same field order, C layout) */
struct bpf_map_attr {
	int type;
	uint32_t key_size;
	uint32_t value_size;
	uint32_t max_ents;
	uint64_t flags;
	uint32_t ifindex;
	uint32_t btf_vmlinux_value_type_id;
	uint32_t btf_id;
	uint32_t btf_key_type_id;
	uint32_t btf_value_type_id;
	uint64_t map_extra;
	uint32_t kernel_bpf_map_id;
	uint64_t gpu_thread_count;
};

/* runtime/include/bpftime_shm.hpp:250-301 (BPF_LINK_CREATE args; 48 B) */
struct bpf_link_create_args {
	uint32_t prog_fd;        /* union { prog_fd; map_fd; } */
	uint32_t target_fd;      /* union { target_fd; target_ifindex; } */
	uint32_t attach_type;    /* BPF_XDP = 37 (runtime/include/bpftime_epoll.h:1158) */
	uint32_t flags;
	uint64_t attach_union[4]; /* attach_type 41: [0] = perf_event.bpf_cookie (link_handler.hpp:25-31) */
};

#define BPFTIME_AMD_BPF_XDP 37
#define BPFTIME_AMD_BPF_PERF_EVENT 41      /* BPFTIME_BPF_PERF_EVENT_ATTACH_TYPE, bpftime_shm.hpp:247 */
#define BPFTIME_AMD_PROG_TYPE_XDP 6        /* bpftime_shm.hpp:144-151 */
#define BPFTIME_AMD_PROG_TYPE_TRACEPOINT 5

/* ---- maps: bpftime_shm.hpp:316-345 ---- */
/* create a map at `fd` (-1: lowest unused fd).  Supported types: HASH (1,
 * fix-size hash, map_handler.cpp:54-58), ARRAY (2), PROG_ARRAY (3, prog
 * fds, prog_array.cpp; the targets of bpf_tail_call, linked into the caller's
 * image at launch), PERF_EVENT_ARRAY (4, perf_event_array_map.cpp: key_size
 * and value_size must be 4, else -1 + EINVAL; max_entries int32 slots, all
 * -1 at first, each the fd of a software perf event.  Lookup returns the
 * slot, update stores the int with the flags ignored, delete stores -1, each
 * -1 / NULL + EINVAL for a key < 0 or >= max_entries; get_next_key: 0 for a
 * NULL key, -1 + ENOENT for the last key, -1 + EINVAL out of range, else key
 * + 1.  A program's bpf_perf_event_output(ctx, map, flags, data, size) writes
 * a sample to the ring of the perf event in the slot of its CPU, see
 * bpftime_amd_perf_event_mmap), PERCPU_HASH (5), PERCPU_ARRAY (6), LRU_HASH (9),
 * LPM_TRIE (11), ARRAY_OF_MAPS (12, map_in_maps.hpp: max_entries int32 slots
 * whatever value_size says, each the fd of an inner map or 0; there is no
 * inner_map_fd, so a slot takes any int.  The host writes slots with
 * bpftime_map_update_elem (the array map's rules: EEXIST for BPF_NOEXIST,
 * E2BIG past the end; it waits for running batches first), reads a 4-byte
 * copy with bpftime_map_lookup_elem (NULL / ENOENT past the end -- the
 * reference dereferences a null pointer there and returns the id as a
 * pointer), delete is EINVAL, get_next_key the array's.  A program's
 * bpf_map_lookup_elem on it yields the slot's fd as the inner map's handle
 * (NULL for an empty slot or a key past the end) for its next map helper
 * call; its update / delete answer -EINVAL.  A slot that names no live map
 * makes those calls answer NULL / -1.  Inner maps must be ARRAY,
 * PERCPU_ARRAY, HASH or PERCPU_HASH: a launch of a program that names an
 * outer map whose slots hold a live map of any other type is refused before
 * any kernel runs, with an error naming the outer fd, slot, inner fd and
 * type), QUEUE (22) and STACK (23: value_size > 0 and max_entries >
 * 0, the key size is not looked at; queue.cpp, stack.cpp), RINGBUF (27),
 * BLOOM_FILTER (30: key_size 0, nr_hashes = map_extra & 0xF with 0 meaning 5,
 * bloom_filter.cpp).  Returns fd or -1 (errno set). */
int bpftime_maps_create(int fd, const char *name, struct bpf_map_attr attr);
/* syscall-side ops (from_syscall = true), bpftime_shm.cpp:115-140 */
const void *bpftime_map_lookup_elem(int fd, const void *key);
long bpftime_map_update_elem(int fd, const void *key, const void *value, uint64_t flags);
long bpftime_map_delete_elem(int fd, const void *key);
int bpftime_map_get_next_key(int fd, const void *key, void *next_key);
/* bpftime_shm.cpp:168-200.  QUEUE / STACK: push appends (flags 0 / BPF_ANY or
 * BPF_EXIST (2), anything else -1 with EINVAL; a full map gives -1 with E2BIG
 * unless the flags are BPF_EXIST, which drops the oldest element -- the
 * queue's head, the stack's bottom -- first); pop removes and copies out the
 * oldest element (queue) or the newest (stack); peek copies without removing;
 * an empty map gives -1 with ENOENT, a NULL value -1 with EINVAL.  On such a
 * map update is a push with the key ignored and the flags not validated
 * (only BPF_EXIST on a full map differs), lookup is a peek (a copy in the
 * thread's lookup buffer), delete a pop that discards, get_next_key -1 with
 * EINVAL.  The ring in device memory is the only copy: the host sees a
 * finished batch's pushes and the next batch sees the host's.  Programs reach
 * these maps through helpers 87 / 88 / 89 and 1 / 2 / 3.  In a parallel batch
 * each QUEUE / STACK map must be add-only (helpers 87 / 2 with flags proven
 * 0), remove-only (88 / 3) or peek-only (89 / 1); a program that mixes these
 * on one map, pushes with non-zero or unproven flags, or reaches 87 / 88 / 89
 * through a map register the loader cannot resolve runs only in
 * EBPF_BATCH_ORDERED batches, which give the reference's sequence exactly;
 * other batches of it are refused at launch.  Across streams a launch that
 * removes from or peeks such a map never overlaps one that adds to one, and
 * an ORDERED launch that touches one (ebpf_exec included) overlaps no other
 * launch that touches one: whichever comes second synchronises the device
 * first.
 * A BLOOM_FILTER takes push (flags must be 0: sets
 * the value's bits, returns 0) and peek (0 when every bit of the value is
 * set, else -1 with ENOENT; *value is not written); pop gives -1 with
 * EOPNOTSUPP.  Every other map type: -ENOTSUP.  lookup / delete /
 * get_next_key on a BLOOM_FILTER fail with EOPNOTSUPP, update is a push (the
 * key, which may be NULL, is ignored). */
long bpftime_map_push_elem(int fd, const void *value, uint64_t flags);
long bpftime_map_pop_elem(int fd, void *value);
long bpftime_map_peek_elem(int fd, void *value);
uint32_t bpftime_map_value_size_from_syscall(int fd);
int bpftime_is_map_fd(int fd);
int bpftime_is_array_map(int fd);
int bpftime_is_prog_fd(int fd);
int bpftime_find_minimal_unused_fd(void);
void bpftime_close(int fd);
/* bpftime_shm.cpp:287-306: a map's creation attributes and name; -1 +
 * ENOENT for a non-map fd */
int bpftime_map_get_info(int fd, struct bpf_map_attr *out_attr, const char **out_name, int *type);
/* bpftime_shm.cpp:347-353 (what the syscall server's mmap64 of an array map
 * fd returns, syscall_context.cpp:915-920): a host view of an ARRAY map's
 * bytes, page aligned, stable until the map is closed.  The device holds the
 * map: host writes to the view reach it before the next launch; the view
 * receives the device bytes when a synchronous batch (EBPF_BATCH_SYNC,
 * ebpf_exec) returns and on bpftime_amd_map_msync.  NULL + EINVAL for other
 * maps. */
void *bpftime_get_array_map_raw_data(int fd);
int bpftime_amd_map_msync(int fd); /* push host writes, wait for the device, pull; 0 / -1 */

/* ---- progs / links (bpftime_shm.hpp:303-309) ---- */
int bpftime_progs_create(int fd, const void *insns, size_t insn_cnt, const char *prog_name, int prog_type);
int bpftime_link_create(int fd, struct bpf_link_create_args *args);
/* ---- perf events (bpftime_shm.hpp:351-380; bpf_perf_event_handler,
 * runtime/src/handler/perf_event_handler.hpp:161-215) ----
 * The targets a link or BPF_PROG_ATTACH names.  A syscall sys_enter or
 * sys_exit tracepoint drives the replay dispatch (bpftime_amd_syscall_dispatch);
 * the other kinds (uprobes, software events) are kept as records so the
 * reference's state imports, exports and links unchanged.
 *
 * A syscall sys_enter tracepoint perf event by syscall number (what
 * perf_event_open of syscalls:sys_enter_<nr>, or raw_syscalls:sys_enter for
 * sys_nr = -1, creates): a new fd, or `fd` when >= 0. */
int bpftime_amd_perf_event_syscall(int fd, int64_t sys_nr);
/* bpftime_shm.hpp:368 (add_tracepoint): by tracepoint id; the id resolves to
 * (syscall number, enter / exit) when a program attaches
 * (bpftime_amd_tracepoint_resolve). */
int bpftime_tracepoint_create(int fd, int pid, int32_t tp_id);
/* bpftime_shm.hpp:356-357: a uprobe / uretprobe record. */
int bpftime_uprobe_create(int fd, int pid, const char *name, uint64_t offset, bool retprobe, size_t ref_ctr_off);
/* bpftime_shm.hpp:371-374: the handler's enabled flag. */
int bpftime_perf_event_enable(int fd);
int bpftime_perf_event_disable(int fd);
int bpftime_is_perf_event_fd(int fd);
/* Any perf event record, with every field the reference's JSON carries
 * (bpftime_shm_json.cpp:66-95, :130-180); get: the record at fd (module_name
 * points into the record). */
struct bpftime_amd_perf_event {
  int type;               /* bpf_event_type: 1 software, 2 tracepoint, 6 uprobe, 7 uretprobe, 1008 override */
  int pid;
  int enabled;
  int32_t tracepoint_id;  /* tracepoint: kernel id, or -1 with sys_nr */
  int64_t sys_nr;         /* tracepoint without an id: the syscall (-1: every syscall) */
  uint64_t offset;        /* uprobe kinds */
  uint64_t ref_ctr_off;
  const char *module_name;
  int cpu;                /* software */
  int32_t sample_type;
  int64_t config;
};
int bpftime_amd_perf_event_record(int fd, const struct bpftime_amd_perf_event *e);
int bpftime_amd_perf_event_get(int fd, struct bpftime_amd_perf_event *e);
/* The ring of a software perf event (type 1; software_perf_event_buffer,
 * perf_event_handler.cpp:235-450): what a program's bpf_perf_event_output
 * (helper 25) writes to through a PERF_EVENT_ARRAY slot that holds the fd.
 * The reference sizes the buffer when the consumer mmaps the perf fd; until
 * then every output is dropped.
 *
 * _mmap gives the perf event a device ring of data_bytes (a power of two, at
 * least 64): u64 data_head and u64 data_tail on a 128-byte line each, then
 * the data bytes, in the map arena.  A second call with the same size does
 * nothing; another size is -1 + EINVAL: a ring cannot be resized.  -1 +
 * EINVAL too for an fd that is no software perf event or a size that is no
 * power of two; -1 + ENOMEM when the arena is exhausted.  Closing the fd and
 * bpftime_amd_reset drop the ring.
 *
 * _fetch is the consumer: it waits for the device, walks the records from
 * data_tail to data_head and copies each whole record -- the 8-byte
 * perf_event_header {u32 type = 9 PERF_RECORD_SAMPLE, u16 misc = 0, u16
 * size}, the u32 data size (size - 12), the data and the padding to 8 -- to
 * `out`, unwrapped and back to back, stopping at the first that does not fit
 * in cap; writes the new data_tail back; returns the record count and sets
 * *used to the bytes written.  A record whose header size is < 8 or larger
 * than the ring drops everything left (copy_next_record_to, :409-450).  0 for
 * a perf event without a ring; -1 for an fd that is no software perf event.
 *
 * _ring_state reads the positions (it waits for the device too) and the
 * ring's size; all 0 before _mmap.  Any out pointer may be NULL. */
int bpftime_amd_perf_event_mmap(int perf_fd, uint64_t data_bytes);
int64_t bpftime_amd_perf_event_fetch(int perf_fd, void *out, uint64_t cap, uint64_t *used);
int bpftime_amd_perf_event_ring_state(int perf_fd, uint64_t *head, uint64_t *tail, uint64_t *data_bytes);
/* bpftime_shm.cpp:249-253 (BPF_PROG_ATTACH): link prog bpf_fd to the perf
 * event: a link fd whose close detaches it; a program linked to a sys_enter
 * tracepoint then runs in bpftime_amd_syscall_dispatch.  -1 + ENOENT when
 * perf_fd is not a perf event or bpf_fd not a program, -1 + EEXIST when a
 * tracepoint id does not resolve, -1 when the device cannot load the
 * program. */
int bpftime_attach_perf_to_bpf(int perf_fd, int bpf_fd);
/* bpftime_shm.cpp:255-260: the same link with an attach cookie, what
 * bpf_get_attach_cookie (174) answers while the linked program runs for this
 * link (bpf_attach_ctx.cpp:380-388 sets it around every callback, syscall
 * tracepoints included).  A link made without one answers 0; so does
 * bpftime_link_create with an attach type other than 41, whose attach_union
 * holds no perf_event.bpf_cookie (link_handler.hpp:25-31), while a type-41
 * link always carries attach_union[0], 0 included.  Same errors as above. */
int bpftime_attach_perf_to_bpf_with_cookie(int perf_fd, int bpf_fd, uint64_t cookie);
/* The same link at `fd` (-1: a fresh one), leaving a link to an unresolvable
 * tracepoint id as a record (the JSON import's add_bpf_link: the reference
 * resolves the id only when its agent attaches). */
int bpftime_amd_link_perf(int fd, int prog_fd, int perf_fd);
/* 1: the link drives a syscall attachment, 0: a record only, -1: not a link. */
int bpftime_amd_link_attached(int fd);

/* Syscall tracepoint ids (attach/syscall_trace_attach_impl/src/
 * syscall_table.cpp:17-98, syscall_trace_attach_private_data.cpp:8-63):
 * the tracefs events directory the ids are read from (default
 * /sys/kernel/tracing/events, or $BPFTIME_AMD_TRACEFS_EVENTS); an id ->
 * (syscall number, enter) with the reference's rules (raw_syscalls sys_enter
 * / sys_exit -> -1; sys_enter_<name> / sys_exit_<name> -> <name>'s number),
 * 0 or -EEXIST; the reverse (-1 when the directory has no such tracepoint);
 * a syscall's number by name (-1 unknown). */
int bpftime_amd_set_tracefs_events(const char *dir);
int bpftime_amd_tracepoint_resolve(int32_t tp_id, int64_t *sys_nr, int *is_enter);
int32_t bpftime_amd_tracepoint_id(int64_t sys_nr, int is_enter);
int64_t bpftime_amd_syscall_nr(const char *name);

/* ---- bpf(2) commands from an interposed loader ----
 * syscall_context::handle_sysbpf's userspace branch
 * (runtime/syscall-server/syscall_context.cpp:429-668): `attr` is the
 * kernel's union bpf_attr.  BPF_MAP_CREATE / BPF_PROG_LOAD / BPF_LINK_CREATE
 * return a new fd; lookups copy the value out (ENOENT when absent); update,
 * delete and get-next-key return the map operation's status; BPF_MAP_FREEZE
 * returns 0; other commands -1 with errno ENOTSUP.
 * BPF_MAP_LOOKUP_BATCH / BPF_MAP_LOOKUP_AND_DELETE_BATCH (attr->batch, the
 * kernel's uapi contract; the reference's handler has no such case) run
 * bpftime_amd_map_dump: the batch token is a u32 cursor, in_batch NULL starts
 * at the beginning, *out_batch receives the next cursor, count is the
 * capacity on input and the entries returned on output.  0, or -1 with ENOENT
 * once the map is exhausted (count is still valid then and may be nonzero);
 * nonzero elem_flags or flags EINVAL; the dump's own errno otherwise. */
long bpftime_amd_handle_sysbpf(int cmd, void *attr, uint32_t size);

/* ---- lddw helpers for the device VM (bpftime_shm.cpp:637-676) ---- */
uint64_t bpftime_amd_map_ptr_by_fd(uint32_t fd); /* the fd itself, ~0 if not a map */
uint64_t bpftime_amd_map_val(uint64_t map_ptr);  /* DEVICE address of the first value */

/* ---- bpftime_amd extensions ---- */
/* device address / byte size of a map's storage (layout: csrc/common.hpp DMap) */
uint64_t bpftime_amd_map_device_ptr(int fd, uint64_t *bytes);
/* raw device-layout copy of the map storage to / from the host */
int bpftime_amd_map_snapshot(int fd, void *out, uint64_t bytes);
int bpftime_amd_map_restore(int fd, const void *in, uint64_t bytes);
/* hash maps: bucket count and device slot geometry */
int bpftime_amd_map_geometry(int fd, uint64_t *nbuckets, uint32_t *slot_size, uint32_t *key_off,
                             uint32_t *val_off, uint32_t *ncpu);
/* (a QUEUE / STACK map: tail - head) */
uint64_t bpftime_amd_map_count(int fd);
/* 1 when this build has a map family for the BPF_MAP_TYPE_* number, else 0
 * (needs no device).  PERF_EVENT_ARRAY (4) is the exception: the family
 * exists and bpftime_maps_create makes one, but this query keeps answering 0
 * for it, as it did before the family was added. */
int bpftime_amd_map_type_supported(uint32_t type);
/* BLOOM_FILTER: the jhash seed (drawn at random per map, as the reference
 * draws it) to *out; a non-NULL `set` installs *set first and zeroes the bit
 * array -- bits set under another seed mean nothing.  0, or -1 (not a Bloom
 * filter). */
int bpftime_amd_bloom_seed(int fd, const uint32_t *set, uint32_t *out);
/* STACK_TRACE (7, stack_trace_map.cpp): bpftime_maps_create needs key_size 4,
 * value_size a multiple of 8 and max_entries > 0, else -1 + EINVAL.  Slot id
 * holds the frames of the stack whose hash is id modulo max_entries, stored by
 * a program's bpf_get_stackid from the batch's recorded stacks (ebpf-vm.h,
 * ebpf_batch::stack_arr).  bpftime_map_lookup_elem returns value_size bytes --
 * the frames, then zeros -- or NULL + ENOENT; update returns -ENOTSUP; delete 0
 * or -1 + ENOENT; get_next_key -1 + ENOTSUP; a NULL key EINVAL.  Every host
 * operation waits for the device first.  _stack_trace_get copies slot id's
 * frames to out (at most cap) and returns the slot's frame count; -1 + ENOENT
 * for an empty slot or an id past the end, -1 + EINVAL when fd is no
 * STACK_TRACE map. */
int bpftime_amd_stack_trace_get(int fd, uint32_t id, uint64_t *out, uint32_t cap);
/* An LPM trie whose device update (ORDERED batch) ran out of the node pool
 * keeps the state from before that batch and reports ENOMEM on every host op
 * and every launch of a program naming a trie until this acknowledges it:
 * 1 when a report was cleared, 0 when there was none, -1 not a map. */
int bpftime_amd_map_ack_error(int fd);
/* virtual CPU count for per-CPU maps and helper 8 (default 64) */
void bpftime_amd_set_ncpu(uint32_t ncpu);
uint32_t bpftime_amd_get_ncpu(void);
/* drop every map / prog / link record and free the device arena */
void bpftime_amd_reset(void);

/* XDP attach surface: enumerate BPF_XDP links -> (link fd, prog fd, ifindex) */
int bpftime_amd_xdp_links(int *link_fds, int *prog_fds, uint32_t *ifindexes, int max);
/* instantiate a prog record into a loaded "mi355x" VM with the default
 * helper groups registered (bpf_attach_ctx.cpp:40-57 equivalent). */
struct ebpf_vm *bpftime_amd_prog_instantiate(int prog_fd, char **errmsg);
/* registers the device helper set (ids 1,2,3,5,7,8,28,44,65,130-133) on a VM */
int bpftime_amd_register_default_helpers(struct ebpf_vm *vm);
/* loader facts: per-lane stack bytes, big (scratch) stack, fused RMW count */
int bpftime_amd_vm_info(const struct ebpf_vm *vm, uint32_t *stack_size, int *big_stack,
                        uint32_t *fused_rmw, uint32_t *n_insns);
void bpftime_amd_set_step_limit(struct ebpf_vm *vm, uint64_t limit);
/* Kernel time (ms) of the vm's last EBPF_BATCH_TIMED batch, waiting for it; -1 when none. */
float bpftime_amd_last_batch_ms(struct ebpf_vm *vm);
/* loads/stores (and array-lookup keys) the loader typed statically for the
 * fast path under the given ctx kind (packet, slot, ctx or stack bases) */
int bpftime_amd_vm_fast_info(const struct ebpf_vm *vm, uint32_t ctx_kind, uint32_t *specialized);
/* The fast path's handler for instruction slot `pc` under the given ctx kind,
 * by name ("SLOW": the C++ tier runs it); NULL when nothing is loaded or pc
 * is past the program. */
const char *bpftime_amd_vm_fast_handler(const struct ebpf_vm *vm, uint32_t ctx_kind, uint32_t pc);
/* Counter adds of the loaded program for one entry form: `deferred` may be
 * summed per wave / block before they reach memory (nothing the unit runs
 * afterwards can observe them), `direct` reach memory at once. */
int bpftime_amd_vm_counter_info(const struct ebpf_vm *vm, uint32_t ctx_kind, uint32_t *deferred, uint32_t *direct);
/* The plan of the vm's last batch launch, as exec_batch chose it (what the
 * BPFTIME_AMD_VERBOSE line prints): read-only, for tests and tools that must
 * know which of the interchangeable mechanisms a launch ran on. */
struct bpftime_amd_launch_info {
  uint64_t units;         /* b->count */
  uint32_t grid, block;   /* blocks, lanes per block (256 or 1024) */
  uint32_t comb_entries;  /* the block's combining table (0: none) */
  uint32_t lcache_sets;   /* the block's lookup cache (0: none) */
  uint32_t stage;         /* bytes of each unit staged in LDS (0: unstaged) */
  uint32_t gregs, gctx;   /* register copy / XDP ctx in global memory (else LDS) */
  uint32_t miss_cap;      /* records per block and partition of the miss log */
  uint32_t tail_lds_depths, tail_lds_words; /* tail-call frames kept in LDS */
  int32_t occupancy;      /* resident blocks per CU */
  uint32_t flush_log;     /* block-end flushes go through the log and k_comb_merge */
  uint32_t miss_log;      /* table misses go through the log and k_miss_merge */
  uint32_t ordered;       /* EBPF_BATCH_ORDERED: one lane, adds straight to memory */
};
/* 0, or -1 when the vm has launched no batch yet. */
int bpftime_amd_vm_last_launch(const struct ebpf_vm *vm, struct bpftime_amd_launch_info *out);

/* ---- handler JSON (csrc/shm_json.cpp) ----
 * The reference's shm export / import format (runtime/include/bpftime_shm.hpp:
 * 237-241, runtime/src/bpftime_shm_json.cpp:103-327): {"<fd>": {"type":
 * "bpf_map_handler" | "bpf_prog_handler" | "bpf_link_handler", "name", "attr"}}.
 * Import recreates maps (in HBM), programs and links at the same fds; a link
 * to an XDP program becomes a BPF_XDP link (the format drops attach types).
 * 0 / -1 (errno, bpftime_amd_last_error). */
int bpftime_import_global_shm_from_json(const char *filename);
int bpftime_export_global_shm_to_json(const char *filename);
int bpftime_import_shm_handler_from_json(int fd, const char *json_string);

/* ---- eBPF ELF objects (csrc/object.cpp) ----
 * The reference opens objects with libbpf (runtime/object/bpftime_object.hpp:
 * bpftime_object_open / _close / _find_program_by_name / _by_secname,
 * bpf_object.cpp:149-260) and relies on libbpf's bpf_object__load for map
 * creation, map / global-data relocation and CO-RE before BPF_PROG_LOAD
 * reaches its syscall server.  These entry points do both: open parses the
 * object (programs, BTF / legacy maps, .bss/.data/.rodata, .rel sections,
 * .BTF.ext CO-RE field relocations against the target BTF); load creates the
 * maps and prog records (bpftime_maps_create / bpftime_progs_create) so the
 * programs run through bpftime_amd_prog_instantiate / bpftime_link_create.
 * Programs are addressed by prog fd (the reference returns bpftime_prog *). */
struct bpftime_object;
/* NULL only if the file cannot be read; parse errors: bpftime_object_error()
 * non-empty and every other call fails */
struct bpftime_object *bpftime_object_open(const char *obj_path);
struct bpftime_object *bpftime_object_open_mem(const void *buf, size_t len, const char *obj_name);
const char *bpftime_object_error(const struct bpftime_object *obj);
/* target BTF for CO-RE (libbpf's btf_custom_path, e.g. the xdp-counter
 * example's base.btf); default: the runtime's own xdp_md layout */
int bpftime_object_load_relocate_btf(struct bpftime_object *obj, const char *btf_path);
int bpftime_object_load_relocate_btf_mem(struct bpftime_object *obj, const void *btf, size_t len);
int bpftime_object_map_count(const struct bpftime_object *obj);
int bpftime_object_map_info(const struct bpftime_object *obj, int idx, const char **name,
                            struct bpf_map_attr *attr);
int bpftime_object_program_count(const struct bpftime_object *obj);
int bpftime_object_program_info(const struct bpftime_object *obj, int idx, const char **name,
                                const char **secname, int *prog_type, size_t *insn_cnt);
/* the relocated instructions of program idx for the given map fds (one per
 * object map, map_info order); returns the instruction count or -1 */
int bpftime_object_program_insns(const struct bpftime_object *obj, int idx, const int *map_fds, void *out,
                                 size_t insn_cap);
/* create the maps (initialised from .data/.rodata) and prog records; 0 / -1 */
int bpftime_object_load(struct bpftime_object *obj);
int bpftime_object_find_program_by_name(const struct bpftime_object *obj, const char *name);      /* prog fd */
int bpftime_object_find_program_by_secname(const struct bpftime_object *obj, const char *secname); /* prog fd */
int bpftime_object_find_map_fd_by_name(const struct bpftime_object *obj, const char *name);
const char *bpftime_object_license(const struct bpftime_object *obj);
void bpftime_object_close(struct bpftime_object *obj);

/* ring buffer consumer (ringbuf::fetch_data, ringbuf_map.cpp): committed
 * records from the consumer position on, each written to `out` as
 * [u32 len][len bytes]; advances the consumer position; returns the record
 * count (-1: not a ring buffer).  Waits for queued batches first. */
int64_t bpftime_amd_ringbuf_fetch(int fd, void *out, uint64_t cap, uint64_t *used);

/* ---- task identity and bpf_trace_printk (Trace and task helpers) ----
 * What bpf_get_current_comm (16) and bpf_get_current_uid_gid (15) answer in
 * this VM's launches.  A VM that never set them answers as the reference
 * does: the basename of the launching process's /proc/self/exe (at most 63
 * bytes) and (getgid() << 32) | getgid().  `comm`: NUL-terminated, at most
 * 63 bytes and the NUL (longer: -1, the VM unchanged); a NULL part stays as
 * it is.  The getter copies 64 bytes of comm (zero from its NUL on). */
int bpftime_amd_vm_set_task(struct ebpf_vm *vm, const char *comm, const uint64_t *uid_gid);
int bpftime_amd_vm_get_task(const struct ebpf_vm *vm, char *comm, uint64_t *uid_gid);
/* What bpf_get_func_ip (173) and bpf_get_attach_cookie (174) answer in this
 * VM's launches (bpf_helper.cpp:684-700): the probed function's address and
 * the attachment's cookie.  Both 0 until set: the reference answers 0 outside
 * any attach callback and for an attachment without a cookie.  The dispatches
 * set them per attachment (bpftime_amd_uprobe_dispatch; a cookie link in
 * bpftime_amd_syscall_dispatch*, where 173 answers 0). */
int bpftime_amd_vm_set_attach(struct ebpf_vm *vm, uint64_t func_ip, uint64_t cookie);

/* bpf_trace_printk (6) is off until the host enables it here (and off again
 * after bpftime_amd_reset): while off it is no default helper
 * (bpftime_amd_register_default_helpers, bpftime_amd_prog_instantiate, the
 * syscall attachments) and a program that calls it is refused at load,
 * naming the helper, as a helper without a device implementation is.  VMs
 * created and programs loaded while it is on keep it.  Returns the previous
 * setting (0 / 1). */
int bpftime_amd_enable_trace_printk(int on);

/* bpf_trace_printk (6) leaves a record in a device log (made when the first
 * program that calls it is loaded; BPFTIME_AMD_TRACE_RECORDS records, default
 * 65536, read then); this formats the records in ticket order, each line
 * exactly what snprintf gives for its format and arguments, NUL-terminated at
 * text + text_off.  Waits for queued batches first.  Delivers only lines that
 * fit whole (max_lines, text_cap) and leaves the rest for the next call; adds
 * the records lost to a full log since the last read to *lost.  Returns the
 * lines delivered; -1 when no log exists.  `unit`: the calling unit's global
 * index (a syscall replay: the record's). */
struct bpftime_amd_trace_line {
  uint64_t unit;
  uint32_t text_off;
  uint32_t text_len;
};
int64_t bpftime_amd_trace_read(struct bpftime_amd_trace_line *lines, uint64_t max_lines, char *text,
                               uint64_t text_cap, uint64_t *lost);

/* ---- syscall tracepoint dispatch (csrc/syscall_dispatch.cpp) ----
 * syscall_trace_attach_impl.cpp:18-95 over recorded syscalls in device memory.
 *
 * attach (create_attach_with_ebpf_callback, :121-166): a program on the
 * sys_enter (is_enter = 1) or sys_exit (0) tracepoint of `sys_nr` in
 * [0, 512), or of every syscall (-1); an attach id, or -1 with errno EINVAL
 * (not a program, sys_nr out of range) or the load error.
 * bpftime_amd_syscall_attach(prog, nr) = bpftime_amd_syscall_attach_ex(prog, nr, 1).
 *
 * Replay records: BPFTIME_AMD_SYSCALL_RECORD (64 B) = trace_event_raw_sys_enter
 * {ent = 0, id, args[6]}; BPFTIME_AMD_SYSCALL_RECORD_FULL (96 B) = that, then
 * trace_event_raw_sys_exit {ent = 0, id, ret} (24 B) at +64, then the
 * calling thread's u64 pid_tgid (tgid << 32 | tid) at +88: the enter ctx and
 * the exit ctx as dispatch_syscall builds them (:57-66, :80-85), each the unit
 * its programs run on in place, and what bpf_get_current_pid_tgid returns to
 * them (bpf_helper.cpp:330-348; 64-B records: the dispatching thread's);
 * BPFTIME_AMD_SYSCALL_RECORD_TIMED (128 B) = the 96-B record, then the
 * recorded clock at sys_enter (u64 ns at +96) and after the call (+104), 16
 * zero bytes: what bpf_ktime_get_ns (bpf_helper.cpp:357-362) returns inside
 * the record's enter / exit callbacks (the replay definition of the clock;
 * other records: the device clock).  Per record
 * (dispatch_syscall :18-95): exit (60) / exit_group (231) run nothing and
 * return ret; the per-syscall enter programs, then the global ones; if one of
 * them called bpf_override_return / bpf_set_retval the record returns that
 * value and its exit programs do not run; else the per-syscall exit programs,
 * then the global ones, and the record returns ret, or the value an exit
 * program set.  Ids outside [0, 512) (the reference indexes its callback
 * arrays with them, undefined there) run only global programs.
 *
 * Order.  The reference runs a call's callbacks on the calling thread, one
 * call after another; threads run side by side.  Two plans give that result:
 *  - program-major (BPFTIME_AMD_DISPATCH_PROGRAMS): each program runs once
 *    over the batch, one lane per record, in the order above; a program that
 *    may store into its ctx runs on a copy of the records, as each reference
 *    callback runs on its own copy (:43-45).  Equal to the per-call order
 *    whenever the attached programs' map effects commute;
 *  - thread-ordered (BPFTIME_AMD_DISPATCH_THREADS): records are grouped by
 *    their recorded pid_tgid (64-B records: one thread, the dispatcher), one
 *    lane per thread walks its records in record order and runs each
 *    record's enter callbacks, the override check and its exit callbacks
 *    before the next record, every callback on a fresh ctx copy: the
 *    reference's own schedule for any programs, threads in parallel.
 * By default the dispatch picks thread-ordered when two attachments may not
 * commute (one writes a map the other reads or writes, or adds to a map the
 * other reads: the loader's map effects, loader.hpp FastForm::map_fx), else
 * program-major.  EBPF_BATCH_ORDERED runs thread-ordered on one lane over
 * every record in record order (the serial reference run).  Thread-ordered
 * dispatch does not run bpf_tail_call (the dispatch fails, named).
 * bpftime_amd_syscall_dispatch_plan(flags) says which plan a dispatch with
 * these flags would take for the current attachments: 1 thread-ordered, 0
 * program-major, -1 on errors.
 *
 * dispatch_records: `out_rets` (device i64 per record, nullable) receives the
 * value dispatch_syscall would return (64-B records have no ret: 0 unless
 * overridden).  64-B records with sys_exit programs attached are refused
 * (EINVAL).  Returns the failed-unit count summed over the programs (a
 * failed callback counts once) with EBPF_BATCH_SYNC, else 0; -1 on errors
 * (bpftime_amd_last_error).  Concurrent dispatches on one stream run one
 * after the other (the dispatch holds the stream's scratch until it has
 * queued its last launch).
 * bpftime_amd_syscall_dispatch(r, n, f, s) = dispatch_records(r, n, 64, NULL, f, s). */
#define BPFTIME_AMD_SYSCALL_RECORD 64
#define BPFTIME_AMD_SYSCALL_RECORD_FULL 96
#define BPFTIME_AMD_SYSCALL_RECORD_TIMED 128
#define BPFTIME_AMD_DISPATCH_THREADS 0x100  /* force the thread-ordered plan */
#define BPFTIME_AMD_DISPATCH_PROGRAMS 0x200 /* force the program-major plan */
int bpftime_amd_syscall_attach(int prog_fd, int64_t sys_nr);   /* attach id or -1 */
int bpftime_amd_syscall_attach_ex(int prog_fd, int64_t sys_nr, int is_enter);
int bpftime_amd_syscall_detach(int id);
int64_t bpftime_amd_syscall_dispatch(const void *records, uint64_t n, uint32_t flags, void *stream);
int64_t bpftime_amd_syscall_dispatch_records(const void *records, uint64_t n, uint32_t record_size,
                                             int64_t *out_rets, uint32_t flags, void *stream);
int bpftime_amd_syscall_dispatch_plan(uint32_t flags);
/* Struct-of-arrays replay records: the same calls as the AoS forms, each
 * field in its own device array, so a dispatch streams only what its
 * programs read (an exit-only dispatch: 32 B per call instead of a 96-B
 * record's three 128-B cache lines' worth).
 *   enter: count x 64 B trace_event_raw_sys_enter {ent = 0, id, args} (NULL
 *          when no sys_enter program is attached: the id comes from exit);
 *   exit:  count x 32 B {trace_event_raw_sys_exit {ent = 0, id, ret} (24 B),
 *          the caller's u64 pid_tgid};
 *   clock: count x 16 B {u64 ns at sys_enter, u64 ns after the call} (the
 *          replayed bpf_ktime_get_ns), or NULL (the device clock).
 * The dispatch runs as bpftime_amd_syscall_dispatch_records over the
 * equivalent 96- / 128-B records (same plans, results and errors). */
struct bpftime_amd_sys_records {
  const void *enter;
  const void *exit;
  const void *clock;
  uint64_t count;
};
int64_t bpftime_amd_syscall_dispatch_soa(const struct bpftime_amd_sys_records *records, int64_t *out_rets,
                                         uint32_t flags, void *stream);

/* ---- uprobe replay (Uprobe replay) ----
 * The reference's third attach family (attach/frida_uprobe_attach_impl):
 * programs attached to a function's entry (uprobe, 6), its return (uretprobe,
 * 7), or in place of it (override 1008, replace 1009).  Here the calls are
 * recorded and replayed: per call the x86-64 struct pt_regs (21 u64, 168 B:
 * di at +112, ax at +80, ip at +128) at entry and at return, the called
 * function's address, and optionally the caller, the clocks and the caller's
 * stack.
 *
 * Which attachments run at a function:
 *  - a function whose first attachment is an override / replace runs only
 *    that one, on the entry registers, and every later attach there fails
 *    with -1 + EEXIST (frida_uprobe_attach_impl.cpp:64-79);
 *  - otherwise its uprobes run at entry and its uretprobes at return, each in
 *    attach order (frida_internal_attach_entry.cpp:221-239); an override /
 *    replace attached after them is kept and never runs, the function being
 *    hooked as a listener (:128-165).
 * bpf_get_func_ip answers `func` inside a uprobe / uretprobe and 0 inside an
 * override / replace (frida_attach_entry.hpp:25-40); bpf_get_attach_cookie
 * the attachment's cookie or 0.  Each program runs on a copy of the record
 * (the reference hands the callback a local pt_regs): stores through r1 never
 * reach `enter` / `leave`.
 *
 * _attach: kind 6 / 7 / 1008 / 1009; `cookie` NULL: none.  An attach id, or -1
 * (EINVAL: not a program / a bad kind / the device cannot load it; EEXIST).
 * _attach_link binds a link record whose target is a uprobe perf event (type
 * 6 / 7 / 1008) to the address its module:offset resolved to in the recording;
 * kind and cookie come from the records.  bpftime_amd_link_attached stays 0
 * for such a link (it drives no syscall attachment); _uprobe_link_bound tells
 * 1 bound / 0 not / -1 no link.  _detach: 0, or -1 + ENOENT. */
#define BPFTIME_AMD_UPROBE 6
#define BPFTIME_AMD_URETPROBE 7
#define BPFTIME_AMD_UPROBE_OVERRIDE 1008
#define BPFTIME_AMD_UREPLACE 1009
#define BPFTIME_AMD_PT_REGS_BYTES 168
int bpftime_amd_uprobe_attach(int prog_fd, uint64_t func, int kind, const uint64_t *cookie);
int bpftime_amd_uprobe_attach_link(int link_fd, uint64_t func);
int bpftime_amd_uprobe_link_bound(int link_fd);
int bpftime_amd_uprobe_detach(int id);
/* The recorded calls: device arrays, one entry per call.  stack_* as
 * ebpf_batch's fields of the same names (include/ebpf-vm.h), indexed by the
 * record. */
struct bpftime_amd_call_records {
  const void *enter;        /* count x 168 B pt_regs at entry, or NULL */
  const void *leave;        /* count x 168 B pt_regs at return, or NULL */
  const uint64_t *func;     /* count: the called function's address */
  const uint64_t *pid_tgid; /* or NULL: the dispatching thread's */
  const void *clock;        /* count x 16 B {ns at entry, ns at return}, or NULL: the device clock */
  const void *stack_arr;
  uint64_t stack_unit_stride, stack_frame_stride;
  const uint32_t *stack_depths;
  uint32_t stack_fixed_depth, stack_max_depth;
  uint64_t count;
};
/* Runs every attachment over the records, by one of two plans.  The plan is
 * the caller's choice and never automatic (the refusal below is behaviour
 * hosts rely on); bpftime_amd_uprobe_dispatch_plan tells it beforehand:
 *   flags                          plan
 *   neither plan flag              program-major; a pair that may not commute is refused
 *   BPFTIME_AMD_DISPATCH_PROGRAMS  the same
 *   BPFTIME_AMD_DISPATCH_THREADS   thread-ordered, whatever the programs share
 *   ... | EBPF_BATCH_ORDERED       thread-ordered with one lane over every record in
 *                                  record order: the serial reference run
 *   both plan flags                -1, EINVAL
 * Program-major: the entry
 * attachments in attach order, then the return attachments.  Per attachment
 * the records of its function are gathered, in record order, into compact
 * 192-B rows {pt_regs, pid_tgid, the phase's clock, record index} and the
 * program runs over them as an EBPF_CTX_UPROBE batch; an attachment that
 * matches no record launches nothing.  An override's bpf_override_return (58)
 * / bpf_set_retval (187) sets bit 0 of out_state[i] and stores the value in
 * out_rets[i]; a replace always does, with the program's r0; every other
 * entry of both arrays keeps what the caller put there.  58 / 187 from a
 * uprobe / uretprobe fail the unit.
 * Program-major order equals the reference's per-call order when the attached
 * programs commute (the syscall dispatch's analysis): two attachments that
 * may not are refused before any launch, the error naming both programs and
 * the map.  A dispatch with a single attachment takes EBPF_BATCH_ORDERED and
 * gives the serial result.  Flags: EBPF_BATCH_SYNC / _ORDERED / _UNCHECKED /
 * _TIMED.
 * Thread-ordered (funclatency's starts[tid] pair, example/tracing/funclatency/
 * funclatency.bpf.c, is the case): the records are grouped by pid_tgid (NULL:
 * one thread owns them all) and one lane per thread walks its calls in record
 * order; per call the entry callbacks of its function run in attach order,
 * then its return callbacks (frida_internal_attach_entry.cpp:221-239), which
 * attachments run at a function decided as above.  Threads are unordered
 * against each other, as in the reference; here a record's return runs right
 * after its entry -- calls recorded inside one another take the event list
 * (bpftime_amd_uprobe_dispatch_events below).  Every callback gets a fresh copy of the
 * phase's pt_regs, the record's caller and clock[i][phase], its attachment's
 * func_ip / cookie and its VM's task identity; counter adds reach memory at
 * once, so a thread's later callback sees its earlier one; out_state /
 * out_rets are written as above, at the record's index.  Nothing is refused
 * for not commuting.  Refused, before any launch: a program that calls
 * bpf_get_stackid / bpf_get_stack (27 / 67); one that touches a QUEUE / STACK
 * map, unless EBPF_BATCH_ORDERED is set; more than 64 running attachments;
 * more than 16 distinct task identities among them.  The host waits on the
 * stream once, for the grouping's thread count.
 * Program-major, the call is never fully asynchronous: per attachment the host waits on the
 * stream once, to read how many records matched (it sizes the rows and the
 * batch from that count, and launches nothing for 0).  Without EBPF_BATCH_SYNC
 * only the last attachment's batch and scatter are left in flight.
 * A replace whose program fails its unit stores 0 and sets bit 0 (a failed
 * exec reports r0 = 0) and is counted; the reference leaves that call's
 * return alone (frida_uprobe_attach_impl.cpp:244-252).
 * Returns the failed callbacks with EBPF_BATCH_SYNC, else 0; -1 with a named
 * error (bpftime_amd_last_error) before any launch for: no records / `func`
 * NULL, an entry attachment without `enter`, a return attachment without
 * `leave`, stack fields that break ebpf_batch's rules, an override / replace
 * attachment without out_state / out_rets. */
int64_t bpftime_amd_uprobe_dispatch(const struct bpftime_amd_call_records *r, uint32_t *out_state,
                                    int64_t *out_rets, uint32_t flags, void *stream);
/* Nested and recursive calls: the thread-ordered plan over an event list.
 * frida's listener runs a function's uprobes in on_enter and its uretprobes in
 * on_leave, on the calling thread, when each happens
 * (frida_internal_attach_entry.cpp:221-239): with f and g probed and f calling
 * g the order is f entry, g entry, g return, f return.  `events` is a device
 * array of n_events words in recorded order, all threads interleaved; a word
 * names a record and a phase.  `r` is the record struct above, unchanged: a
 * record still holds both register sets, func, pid_tgid and clock[i] = {entry
 * ns, return ns}.
 *  - Plan: thread-ordered only.  `flags` must carry
 *    BPFTIME_AMD_DISPATCH_THREADS; EBPF_BATCH_ORDERED may be added (one lane
 *    walks the whole list in list order: the serial reference run); without the
 *    flag, or with BPFTIME_AMD_DISPATCH_PROGRAMS, -1 + EINVAL, the error naming
 *    the flag.  bpftime_amd_uprobe_dispatch_plan answers for these flags.
 *  - An event belongs to thread pid_tgid[record] (NULL: one thread owns every
 *    event); both phases of a call run on the calling thread.  Lane t walks
 *    thread t's events in list order; threads are unordered against each other.
 *  - Per event: phase 0 runs the entry callbacks of func[record], phase 1 its
 *    return callbacks -- which attachments, and in which order, as above (a
 *    function hooked by replacement runs its override / replace at phase 0 and
 *    nothing at phase 1).  Every callback gets a fresh copy of enter[record] /
 *    leave[record] with r2 = 168, clock[record][phase] (NULL: the device
 *    clock), the record's caller, its attachment's func_ip / cookie and its
 *    VM's identity; 58 / 187 and a replace's r0 write out_state[record] /
 *    out_rets[record] as above; counter adds reach memory at once.
 *  - No pairing is required or checked: the replay runs what the list says.  A
 *    record may appear with its entry only (a call that never returned), with
 *    its return only (entered before recording began) or not at all -- then
 *    nothing runs for it and its out_* entries keep the caller's values; the
 *    same event twice runs twice.
 *  - The flat list E(0,0), E(0,1), E(1,0), E(1,1), ... gives exactly what
 *    bpftime_amd_uprobe_dispatch with BPFTIME_AMD_DISPATCH_THREADS gives on the
 *    same records.
 * Refused with -1 and a named error, before any callback runs and with no map
 * changed: `events` NULL or n_events 0; count >= 2^31 (a word holds a 31-bit
 * record index); n_events >= 2^32; an event whose record index is >= count
 * (counted on the device and read in the host's one wait, the grouping's --
 * with one thread, a wait of its own; the error tells how many); and every
 * refusal of the thread-ordered plan and of the record checks above.
 * The return value and EBPF_BATCH_SYNC / _UNCHECKED / _TIMED as the
 * thread-ordered dispatch's; after a timed call bpftime_amd_uprobe_last_ms
 * tells the grouping's time (the key pass included), the replay launch's, and
 * n_events as the rows. */
#define BPFTIME_AMD_CALL_EVENT(record, phase) (((uint32_t)(record) << 1) | ((uint32_t)(phase) & 1u))
int64_t bpftime_amd_uprobe_dispatch_events(const struct bpftime_amd_call_records *r,
                                           const uint32_t *events, uint64_t n_events,
                                           uint32_t *out_state, int64_t *out_rets,
                                           uint32_t flags, void *stream);
/* The plan a dispatch with these flags takes for the current attachments: 1
 * thread-ordered, 0 program-major, -1 with the named error such a dispatch
 * would give (both plan flags, a pair that may not commute, a thread-ordered
 * refusal). */
int bpftime_amd_uprobe_dispatch_plan(uint32_t flags);
/* The tier that ran the callbacks of the calling host thread's most recent
 * thread-ordered dispatch (BPFTIME_AMD_DISPATCH_THREADS), of syscall records,
 * of recorded calls or of an event list: 1 the asm tier (LDS
 * stacks, the hand-written threaded code), 0 the C++ tier, -1 when this thread
 * has queued none.  Thread-local; set when the launch is queued.  Both tiers
 * compute the same: this is a diagnostic for tests and measurements
 * (BPFTIME_AMD_SEQ_ASM=1 / 0 forces a tier; a program with a stack of more than
 * 64 B keeps the whole dispatch in the C++ tier either way). */
int bpftime_amd_last_seq_tier(void);
/* The last EBPF_BATCH_TIMED dispatch, summed over its attachments: the time of
 * the count + scan launches, of the gather launches (ms, stream events), and
 * the rows gathered.  After a thread-ordered dispatch: the thread grouping's
 * time, the replay launch's, and the records.  Any out pointer may be NULL. */
int bpftime_amd_uprobe_last_ms(float *count_ms, float *gather_ms, uint64_t *rows);

/* ---- XDP completion (XDP completion; csrc/xdp_complete.cpp) ----
 * What a runner does after an EBPF_CTX_XDP batch, on the device: the batch's
 * per-unit outputs become one descriptor list per verdict, each in unit order
 * (a flow's packets leave in the order they came), and optionally the frames
 * of chosen lists are packed into one buffer for a single copy to the host.
 * Queue it on the batch's stream, after the batch; no sync is needed between.
 *
 * Unit i's frame address is descs[i].addr, or i * stride when descs is NULL
 * (strided mode).  After the program its frame is [addr + off, addr + off +
 * len): off = data_off_out[i] (0 without the array), len = len_out[i]
 * (descs[i].len without it); strided mode needs both arrays.  Its chunk is
 * [base, base + stride), base = addr - addr % stride.
 *
 * Class of a unit: its verdict when that is <= 4 (XDP_ABORTED 0, DROP 1, PASS
 * 2, TX 3, REDIRECT 4), 0 for every other value; and 0 whatever the verdict
 * when the frame does not lie inside its chunk or the chunk does not lie
 * inside [0, umem_bytes) (64-bit arithmetic that does not wrap; such a unit
 * is `confined`, below).
 *
 * List c (class c): out[c][k] and index_out[c][k] describe the k-th unit of
 * class c in ascending unit index, for k < cap[c]; nothing is written at or
 * past cap[c]; either pointer may be NULL (both: the class is only counted).
 * index_out holds the unit index.  The entry of a unit whose class is in
 * frame_mask (bit c = class c) is its frame {addr + off, len, options}
 * (options copied from descs[i], 0 in strided mode); of any other unit, and of
 * every confined unit, the chunk to hand back to the FILL ring {base, 0, 0} --
 * or {addr, 0, 0} when the chunk is outside the umem.  counts (device u32[5],
 * may be NULL) receives the classes' totals, not clamped to cap.
 *
 * Gather (gather non-NULL; a device or pinned-host pointer): the units whose
 * class is in gather_mask (a subset of frame_mask), that are not confined and
 * whose len <= gather_stride, form one merged list in ascending unit index.
 * Its k-th frame's len bytes are copied from umem + addr + off to gather + k *
 * gather_stride, gather_descs[k] = {k * gather_stride, len, options} and
 * gather_index[k] = the unit, for k < gather_cap (either array may be NULL).
 * Bytes [len, gather_stride) of a slot and slots at or past the list's length
 * or gather_cap are not written.  gather_count (device u32, may be NULL): the
 * list's length, not clamped.  A unit left out for len > gather_stride is
 * counted in gather_skipped (device u32, may be NULL); it stays in its class
 * list.
 *
 * BPFTIME_AMD_XDP_COMPLETE_SYNC: the call waits for the stream and writes the
 * five totals to host_counts (host u32[5]) and, when non-NULL, the gather
 * list's length and the skipped count to host_gather (host u32[2]).
 *
 * Returns 0, or -1 with a named bpftime_amd_last_error(), before anything is
 * launched, for: args NULL or a struct_size that is not sizeof(struct
 * bpftime_amd_xdp_complete_args); count >= 2^32; verdicts NULL; stride 0; an
 * array that is not aligned to its element (4 B, descriptors 8 B); strided
 * mode without data_off_out and len_out, or with count * stride >= 2^63;
 * frame_mask with bits past the five classes; gather_mask outside frame_mask;
 * gather without gather_stride or without umem; gather_cap * gather_stride >=
 * 2^63; SYNC without host_counts.  count 0 succeeds with zero counts. */
#define BPFTIME_AMD_XDP_COMPLETE_SYNC 0x1
#define BPFTIME_AMD_XDP_CLASSES 5
#define BPFTIME_AMD_XDP_FRAME_MASK_DEFAULT 0x1c /* PASS | TX | REDIRECT */
struct bpftime_amd_xdp_complete_args {
  uint32_t struct_size;       /* sizeof(struct bpftime_amd_xdp_complete_args) */
  uint32_t flags;             /* BPFTIME_AMD_XDP_COMPLETE_* */
  /* the finished batch (bpftime_amd_xdp_complete_from_batch fills these) */
  uint64_t count;
  const uint32_t *verdicts;
  const struct ebpf_xdp_desc *descs;
  const int32_t *data_off_out;
  const uint32_t *len_out;
  const void *umem;           /* device base of the frames (the batch's data); read by the gather only */
  uint64_t stride;            /* the umem chunk size, or the slot stride */
  uint64_t umem_bytes;
  void *stream;
  /* the lists */
  struct ebpf_xdp_desc *out[BPFTIME_AMD_XDP_CLASSES];
  uint32_t *index_out[BPFTIME_AMD_XDP_CLASSES];
  uint64_t cap[BPFTIME_AMD_XDP_CLASSES];
  uint32_t frame_mask;
  uint32_t gather_mask;
  uint32_t *counts;
  uint32_t *host_counts;
  /* the gather */
  void *gather;
  uint64_t gather_stride;
  uint64_t gather_cap;
  struct ebpf_xdp_desc *gather_descs;
  uint32_t *gather_index;
  uint32_t *gather_count;
  uint32_t *gather_skipped;
  uint32_t *host_gather;
};
int bpftime_amd_xdp_complete(const struct bpftime_amd_xdp_complete_args *args);
/* Zeroes *args and fills struct_size, the batch half (count, verdicts, descs,
 * data_off_out, len_out, umem, stride, umem_bytes -- count * stride in strided
 * mode -- and stream) from an EBPF_CTX_XDP batch, and frame_mask with the
 * default, so the two calls cannot disagree.  -1 (named) for a NULL pointer or
 * a batch of another ctx kind. */
int bpftime_amd_xdp_complete_from_batch(const struct ebpf_batch *batch, struct bpftime_amd_xdp_complete_args *args);
/* Units per workgroup tile of the partition kernels, and tiles per pass of
 * the tile-offset scan (for tests that pick sizes around them). */
uint32_t bpftime_amd_xdp_complete_tile(void);
uint32_t bpftime_amd_xdp_complete_scan_tiles(void);

/* ---- map dump and drain (Map dump and drain; csrc/map_dump.cpp) ----
 * Reads a map out in one call: up to `cap` entries from the cursor `start`,
 * as dense key and value arrays, in the order a bpftime_map_get_next_key walk
 * yields them.  A hash table is compacted on the device (csrc/map_dump.hip:
 * count, scan, scatter; no atomics, no workgroup waiting on another), so only
 * the entries returned cross to the caller.
 *
 * HASH, PERCPU_HASH, LRU_HASH: the cursor is a bucket index and end = the
 * bucket count.  The entries are the live buckets (state word 1) with index >=
 * start, in index order, the first cap of them; empty buckets and LRU
 * tombstones are skipped.  next = the index of the first live bucket not
 * returned, or end when every live bucket at or after start was returned.
 * ARRAY, PERCPU_ARRAY: the cursor is an element index, end = max_entries; the
 * entries are elements start .. start + cap - 1 (clipped at end), the keys
 * their u32 indices; next = start + count.
 * A value is the syscall side's view, bpftime_map_value_size_from_syscall(fd)
 * bytes: for a per-CPU map all ncpu values, contiguous.
 *
 * keys / values may be host or device memory (the copy is hipMemcpyDefault)
 * and either may be NULL: that output is skipped, the entries still count
 * (and with BPFTIME_AMD_DUMP_DELETE are still deleted).  start == end returns
 * 0 with count 0 and next = end; cap == 0 returns 0 with count 0 and next =
 * start, without a launch.
 *
 * A plain dump changes nothing in the map: not the slots, not the element
 * counter, not an LRU map's stamps (a dump is not a use, as the kernel's
 * batch lookup refreshes no recency).
 *
 * BPFTIME_AMD_DUMP_DELETE (HASH, PERCPU_HASH): each returned entry's state
 * word becomes 0 (key and value bytes stay), the element counter drops by
 * count and the lookup index is invalidated; no launch that trusts its lookup
 * cache is running by then.  The map is left exactly as count calls of
 * bpftime_map_delete_elem on the returned keys leave it when each finds its key
 * (last returned first: in bucket order a delete of an earlier bucket of a
 * probe run can orphan a later key of the run, whose own delete then finds
 * nothing; the drain clears exactly the buckets it returned).  On ARRAY /
 * PERCPU_ARRAY it is EINVAL, as their delete.  On LRU_HASH it is ENOTSUP:
 * tombstones, the tombstone counter and compaction stay with the map's own
 * delete; drain an LRU map with bpftime_map_delete_elem.
 *
 * The call is synchronous: it takes the runtime lock and waits for the device
 * first, so a batch on any stream has finished and its deferred counter adds
 * are in the table.  Like every host-side map operation it must not race a
 * batch launched meanwhile from another thread.
 *
 * 0, or -1 with errno and bpftime_amd_last_error: EINVAL (NULL args -- before
 * anything else --, unknown flag bits, start > end, DELETE on an array),
 * ENOENT (fd is no map), ENOTSUP (every other map type, naming the type; DELETE
 * on LRU_HASH), ENOMEM / EIO (the device).  The checks of args, flags and fd
 * need no device. */
#define BPFTIME_AMD_DUMP_DELETE 1u /* also remove every entry returned */
struct bpftime_amd_map_dump_args {
  int fd;
  uint32_t flags; /* 0 or BPFTIME_AMD_DUMP_DELETE; any other bit: EINVAL */
  uint64_t start; /* in: cursor, 0 = from the beginning */
  uint64_t cap;   /* in: entries keys / values have room for */
  void *keys;     /* out: count * key_size bytes, dense; host or device memory; may be NULL */
  void *values;   /* out: count * bpftime_map_value_size_from_syscall(fd) bytes, dense; may be NULL */
  uint64_t count; /* out: entries returned (<= cap) */
  uint64_t next;  /* out: cursor to pass as start to continue */
  uint64_t end;   /* out: the cursor value that means "nothing left" */
};
int bpftime_amd_map_dump(struct bpftime_amd_map_dump_args *args);
/* Buckets per workgroup tile of the dump kernels, and tiles per pass of the
 * tile-offset scan (for tests that pick sizes around them). */
uint32_t bpftime_amd_map_dump_tile(void);
uint32_t bpftime_amd_map_dump_scan_tiles(void);

/* ---- attach plugins (attach/base_attach_impl/base_attach_impl.hpp:24-71,
 * attach/simple_attach_impl/simple_attach_impl.cpp:7-55; csrc/attach.cpp) ----
 * An attach entry is a program loaded on the device.  bpftime_amd_attach_run
 * has the shape of ebpf_run_callback, int(void *memory, size_t memory_size,
 * uint64_t *return_value), with the entry as a leading context argument, so a
 * base_attach_impl can bind it as its callback: one unit,
 * bpftime_prog_exec's contract.  bpftime_amd_attach_run_batch runs the entry
 * over a device batch (ebpf_exec_batch's contract). */
struct bpftime_amd_attach;
struct bpftime_amd_attach *bpftime_amd_attach_create(int prog_fd, int ctx_kind); /* ctx_kind -1: from the prog type */
int bpftime_amd_attach_run(void *attach, void *memory, size_t memory_size, uint64_t *return_value);
int bpftime_amd_attach_run_batch(struct bpftime_amd_attach *attach, const struct ebpf_batch *batch);
void bpftime_amd_attach_destroy(struct bpftime_amd_attach *attach);
/* simple_attach_impl over device batches: create an impl for one attach
 * type with a callback; attach one program (a second attach, or a mismatched
 * type, fails: -1); trigger calls cb(attach-time argument, trigger argument,
 * the attach entry) and returns its result, or 1 when nothing is attached;
 * detach by the id attach returned. */
typedef int (*bpftime_amd_simple_callback)(const char *argument, void *trigger_argument,
                                           struct bpftime_amd_attach *attach);
int bpftime_amd_simple_attach_impl_create(int attach_type, bpftime_amd_simple_callback cb);
int bpftime_amd_simple_attach(int impl, int prog_fd, int ctx_kind, const char *argument, int attach_type);
int bpftime_amd_simple_detach(int impl, int id);
int bpftime_amd_simple_trigger(int impl, void *trigger_argument);
int bpftime_amd_simple_attach_impl_destroy(int impl);

/* ---- host merge of per-GPU map shards ---- */
/* acc += shard - init over u64 words (array counters, additive rule) */
int bpftime_amd_merge_delta_u64(void *acc, const void *init, const void *shard, uint64_t bytes);
/* The same rule counter by counter at `width` bytes (1, 2, 4, 8): a u32
 * counter's combined delta wraps at 2^32 instead of carrying into the next
 * field.  -1 when bytes is not a multiple of width. */
int bpftime_amd_merge_delta(void *acc, const void *init, const void *shard, uint64_t bytes, uint32_t width);

/* ---- device utilities (HIP runtime plumbing for callers without one) ---- */
int bpftime_amd_device_count(void);
int bpftime_amd_hip_runtime_version(void);  /* hipRuntimeGetVersion of the runtime this library runs on, -1 on error */
/* Experiment counters (BPFTIME_AMD_DBG=512: hash lookup-cache hit lanes, miss lanes): up to n
 * u64 into out after the device is idle, zeroed when reset; the count or -1. */
int bpftime_amd_dbg_counters(uint64_t *out, int n, int reset);
int bpftime_amd_set_device(int dev);
void *bpftime_amd_dev_alloc(uint64_t bytes);
void bpftime_amd_dev_free(void *p);
int bpftime_amd_memcpy_htod(void *dst, const void *src, uint64_t bytes);
int bpftime_amd_memcpy_dtoh(void *dst, const void *src, uint64_t bytes);
/* async copies on a stream (host side must be pinned for overlap) */
int bpftime_amd_memcpy_htod_async(void *dst, const void *src, uint64_t bytes, void *stream);
int bpftime_amd_memcpy_dtoh_async(void *dst, const void *src, uint64_t bytes, void *stream);
void *bpftime_amd_stream_create(void); /* non-blocking hipStream_t */
void bpftime_amd_stream_destroy(void *stream);
int bpftime_amd_stream_sync(void *stream);
int bpftime_amd_memset(void *dst, int v, uint64_t bytes);
int bpftime_amd_sync(void);
void *bpftime_amd_host_alloc(uint64_t bytes); /* pinned */
void bpftime_amd_host_free(void *p);
/* events on a stream: returns elapsed ms between start/stop records */
void *bpftime_amd_event_create(void);
void bpftime_amd_event_destroy(void *ev);
int bpftime_amd_event_record(void *ev, void *stream);
/* work queued on `stream` after this waits for the event's last record */
int bpftime_amd_stream_wait_event(void *stream, void *ev);
float bpftime_amd_event_elapsed_ms(void *start, void *stop);
const char *bpftime_amd_last_error(void);

/* ---- synthetic inputs (seeded splitmix64) ---- */
/* word k of the stream = splitmix64 output #k for `seed`:
 *   z = seed + (k+1)*0x9E3779B97F4A7C15; z = (z^(z>>30))*0xBF58476D1CE4E5B9;
 *   z = (z^(z>>27))*0x94D049BB133111EB; z ^= z>>31 */
/* n packets in `stride`-byte device slots (first `len` bytes random, bytes
 * 12..13 = 0x08 0x00); unit i uses words of stream index first+i. */
int bpftime_amd_gen_xdp(void *dev, uint64_t n, uint64_t stride, uint32_t len, uint64_t seed,
                        uint64_t first, void *stream);
/* config 3 frames (gen.py flow_packets): `cdf` = device copy of the Zipf
 * CDF (nflows doubles, computed on the host); per-unit lengths to `lens`. */
int bpftime_amd_gen_flow(void *dev, uint32_t *lens, uint64_t n, uint64_t stride, uint64_t seed,
                         uint64_t first, const double *cdf, uint32_t nflows, void *stream);
/* config 5 records (gen.py syscall_records), 64 B each. */
int bpftime_amd_gen_syscall(void *dev, uint64_t n, uint64_t seed, uint64_t first, const double *cdf,
                            uint32_t support, void *stream);
/* 96-B replay records (gen.py syscall_records_full): config 5's enter record
 * (id -1 for 0.5 %), then the exit ctx {0, id, ret}, then a pid_tgid. */
int bpftime_amd_gen_syscall_full(void *dev, uint64_t n, uint64_t seed, uint64_t first, const double *cdf,
                                 uint32_t support, void *stream);
/* The same calls as struct-of-arrays records (bpftime_amd_syscall_dispatch_soa):
 * enter (n x 64 B, may be NULL) and exit (n x 32 B {exit ctx, pid_tgid}). */
int bpftime_amd_gen_syscall_soa(void *enter, void *exit, uint64_t n, uint64_t seed, uint64_t first,
                                const double *cdf, uint32_t support, void *stream);
/* Static LDS bytes of the interpreter kernel for a launch shape (its
 * attribute; the restated sum without a device): with the dynamic part
 * (common.hpp dyn_lds_for) what a block needs of the CU's 160 KiB. */
size_t bpftime_amd_static_lds(uint32_t kind, bool big_stack, bool gregs, uint32_t block);
/* Dynamic + static LDS bytes of an interpreter block (ctx kind, 512-B scratch
 * stack, per-lane stack bytes, combining-table entries, lookup-cache sets,
 * ctx in LDS, register copy in global memory, lanes): a launch whose block
 * needs more than 160 KiB fails with a named error (vm_upkeep.cpp). */
size_t bpftime_amd_lds_bytes(uint32_t kind, bool big_stack, uint32_t stack_size, uint32_t comb_entries,
                             uint32_t lcache_sets, bool ctx_lds, bool gregs, uint32_t block);

#ifdef __cplusplus
}
#endif
#endif
