// bpftime_amd: a loaded program's device image -- the decoded program, its
// threaded forms linked per launch configuration, and the tail-call image
// relinked when a prog array changes.
#include "vm_impl.hpp"

namespace bpftime_amd {
// The asm tier dispatches straight into its handlers (gen_fast.py: direct
// dispatch): an FInsn names its handler by the handler's offset from the
// asm's handler base, not by its id.  The offsets are assembly-time
// constants of each of the two asm variants (the C++ tier's register copy in
// LDS or in global memory, k_interp G); the kernel reports them once per
// process (its query entry), and every linked program is translated from
// handler ids to them.  Handlers are laid out in id order, so the offsets
// must rise: anything else fails the link.
static std::mutex g_xlat_mu;
static std::vector<uint32_t> g_xlat[2];
static const std::vector<uint32_t> *fast_xlat(bool greg) {
  std::lock_guard<std::mutex> g(g_xlat_mu);
  std::vector<uint32_t> &t = g_xlat[greg ? 1 : 0];
  if (!t.empty()) return &t;
  uint32_t *d = nullptr;
  std::vector<uint32_t> h(F_COUNT, ~0u);
  bool ok = hipMalloc((void **)&d, 4 * F_COUNT) == hipSuccess &&
            hipMemset(d, 0xff, 4 * F_COUNT) == hipSuccess &&
            bpftime_amd_launch_fast_xlat(CTX_RAW, false, greg, false, d, nullptr) == hipSuccess &&
            hipDeviceSynchronize() == hipSuccess &&
            hipMemcpy(h.data(), d, 4 * F_COUNT, hipMemcpyDeviceToHost) == hipSuccess;
  if (d) hipFree(d);
  for (uint32_t i = 1; ok && i < F_COUNT; i++) ok = h[i] > h[i - 1] && h[i] < (1u << 24);
  if (!ok) return nullptr;
  t = std::move(h);
  return &t;
}

const FInsn *Image::linked(bool greg, bool xdp, uint32_t head, uint32_t stage, bool ordered, int32_t unwind_idx,
                         uint32_t lc_sets, int32_t pid_off, bool no_kldx, RecOffs rec) {
  std::lock_guard<std::mutex> g(link_mu);
  // (the helpers with asm handlers an unwind index changes: lookup, pid_tgid)
  const bool uw = unwind_idx == 1, uwp = unwind_idx == 14;
  const uint32_t po = pid_off > 0 && pid_off < 256 && !uwp ? (uint32_t)pid_off : 0;
  const uint64_t key = ((uint64_t)xdp << 63) | ((uint64_t)ordered << 62) | ((uint64_t)uw << 61) |
                       ((uint64_t)(lc_sets & 0x1fff) << 47) | ((uint64_t)stage << 40) | ((uint64_t)po << 32) |
                       (stage ? head : 0);
  const bool uwu = unwind_idx == 2;  // (map_update_elem's asm handler)
  // (rec: the ctx copy's caller / clock offsets, both below 256)
  const auto lk = std::make_pair(key, (uint32_t)no_kldx | ((uint32_t)(rec.pid != 0) << 1) | ((uint32_t)uwu << 2) |
                                          ((uint32_t)greg << 3) | ((rec.pid & 0xffu) << 8) |
                                          ((rec.clock & 0xffu) << 16));
  auto it = links.find(lk);
  if (it != links.end()) return it->second;
  std::vector<FInsn> out;
  link_fast(xdp ? fx : fr, head, stage, ordered, prog.prog, out, uw ? 1 : uwu ? 2 : -1, lc_sets, po, no_kldx,
            rec);
  if (getenv("BPFTIME_AMD_DUMP_FAST"))  // the linked threaded form, one FInsn a line
    for (size_t i = 0; i < out.size(); i++)
      fprintf(stderr, "bpftime_amd: fast %3zu %-18s w1 %08x imm %llx dst %u src %u tgt %u aux %x\n", i,
              fop_name((out[i].hoff - 4) / 4), out[i].w1, (unsigned long long)out[i].imm, out[i].dst_x2 / 2,
              out[i].src_x2 / 2, out[i].target / kFastInsnBytes, (unsigned)out[i].aux);
  // handler ids -> the variant's handler offsets (this FInsn's and, in
  // w1 bits 8.., the next one's)
  const std::vector<uint32_t> *xl = fast_xlat(greg);
  if (!xl) return nullptr;
  // jumps also carry their target's handler offset (gen_fast.py
  // jump_taken): w2 for JA and register compares (their imm is unused),
  // w5 for immediate compares (their src is unused)
  std::vector<uint32_t> jt(out.size(), ~0u);
  for (size_t i = 0; i < out.size(); i++) {
    const uint32_t id = (out[i].hoff - 4) / 4;
    if (id != F_JA && (id < F_J64_EQ_R || id > F_J32_SLE_I)) continue;
    const size_t t = out[i].target / kFastInsnBytes;
    jt[i] = t < out.size() ? (out[t].hoff - 4) / 4 : (uint32_t)F_SLOW;
    if (jt[i] >= F_COUNT) return nullptr;
  }
  for (FInsn &x : out) {
    const uint32_t id = (x.hoff - 4) / 4, nid = ((x.w1 >> 8) - 4) / 4;
    if (x.hoff < 4 || id >= F_COUNT || (x.w1 >> 8) < 4 || nid >= F_COUNT) return nullptr;
    x.hoff = (*xl)[id];
    x.w1 = (x.w1 & 0xffu) | ((*xl)[nid] << 8);
    const size_t i = &x - out.data();
    if (jt[i] == ~0u) continue;
    static_assert((F_J64_EQ_I - F_J64_EQ_R) == 1 && (F_J32_SLE_I - F_J64_EQ_R) % 2 == 1,
                  "jump handlers alternate register / immediate forms");
    if (id != F_JA && (id - F_J64_EQ_R) % 2 == 1)
      x.src_x2 = (*xl)[jt[i]];
    else
      x.imm = (int64_t)(*xl)[jt[i]];
  }
  FInsn *d = nullptr;
  const size_t bytes = out.size() * sizeof(FInsn);
  if (hipMalloc((void **)&d, bytes) != hipSuccess) return nullptr;
  if (hipMemcpy(d, out.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    hipFree(d);
    return nullptr;
  }
  links[lk] = d;
  return d;
}
// device copy of the decoded program + both threaded forms
int Image::upload(LoadOut &&out, std::string &err) {
  if (out.trace_printk && trace_log_ensure() < 0) {
    err = "trace log: device alloc failed";
    return -1;
  }
  build_fast(out, true, fx);
  build_fast(out, false, fr);
  out.comb_entries = (fx.needs_comb || fr.needs_comb) ? kComb : 0;
  const size_t bytes = out.prog.size() * sizeof(DInsn);
  if (hipMalloc((void **)&d_prog, bytes) != hipSuccess ||
      hipMemcpy(d_prog, out.prog.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    err = "device upload failed";
    return -1;
  }
  prog = std::move(out);
  return 0;
}

int Mi355xVm::load_code(const void *code, size_t code_len) {
  if (code_len % 8 != 0) {
    error = "Length of code must be a multiple of 8";
    return -1;
  }
  if (loaded) {
    error = "code has already been loaded into this VM. Use ebpf_unload_code() if you need to reuse this VM";
    return -1;
  }
  LoadOut out;
  std::string err;
  int rc = load_program((const RawInsn *)code, code_len / 8, helper_id_map, helper_names, lddw, out, err);
  if (rc < 0) {
    error = err;
    return rc;
  }
  if (rt().ensure_device() < 0) {
    error = "no HIP device: " + rt().last_error;
    return -1;
  }
  if (!d_err && hipMalloc((void **)&d_err, 4 * kErrSlots) != hipSuccess) {
    error = "device alloc failed";
    return -1;
  }
  has_tail = out.tail_call;
  base_stack = out.big_stack ? kStackSize + 1 : out.stack_size;
  auto im = std::make_shared<Image>();
  if (im->upload(std::move(out), error) < 0) return -1;
  raw.assign((const RawInsn *)code, (const RawInsn *)code + code_len / 8);
  {
    std::lock_guard<std::mutex> g(img_mu);
    img = std::move(im);
  }
  loaded = true;
  return 0;
}

// Link the loaded program with the programs its prog arrays can reach:
// the arrays it loads by fd (lddw src 1), the targets they name, and
// transitively the arrays those targets load.  One image, the targets
// appended (raw jumps are relative, so they need no relocation) with their
// exits turned into kRetHelper calls, plus a prog fd -> entry pc table.  A
// target that does not load alone is left out, so tail calls to it return
// -1 like a failed bpftime_prog_load (bpf_helper.cpp:623-628); the reason
// is kept in link_note.  Called with img_mu held.
int Mi355xVm::link_tail_image_locked() {
  Runtime &r = rt();
  if (img && img->gen == r.prog_gen && img->d_tail_entry) return 0;
  std::map<size_t, size_t> hm = helper_id_map;
  std::map<size_t, std::string> names = helper_names;
  for (uint32_t id : {1u, 2u, 3u, 5u, 7u, 8u, 12u, 28u, 44u, 65u, 87u, 88u, 89u, 130u, 131u, 132u, 133u, 189u})
    if (!hm.count(id)) hm[id] = 63;  // the runtime's helper groups (bpf_helper.cpp:606-620)
  // prog arrays named by lddw src 1 in `code`
  auto arrays_of = [&](const RawInsn *code, size_t n, std::set<int32_t> &out) {
    // (the fd as BPF_PSEUDO_MAP_FD, or as a plain 64-bit immediate the way
    // runtime/unit-test/tailcall/test_user_to_user_tailcall.cpp loads it)
    for (size_t i = 0; i + 1 < n; i++)
      if (code[i].code == 0x18) {
        const uint64_t v = (uint64_t)(uint32_t)code[i].imm | ((uint64_t)(uint32_t)code[i + 1].imm << 32);
        const bool as_fd = code[i].src == 1 || (code[i].src == 0 && v < kMaxFds);
        const int32_t fd = code[i].imm;
        if (as_fd && fd >= 0 && fd < (int32_t)kMaxFds && r.kind[fd] == HKind::MAP &&
            r.maps[fd].type == MT_PROG_ARRAY)
          out.insert(fd);
        i++;
      }
  };
  // the prog arrays each program loads, and the targets each array names
  std::map<int32_t, std::set<int32_t>> arrays_of_prog;  // target prog fd -> arrays
  std::map<int32_t, std::vector<int32_t>> slots_of;     // array fd -> target prog fds
  std::map<int32_t, std::vector<int32_t>> slot_fds;     // array fd -> its slots (prog fds) at link time
  std::set<int32_t> root_arrays, pending;
  arrays_of(raw.data(), raw.size(), root_arrays);
  pending = root_arrays;
  link_note.clear();
  while (!pending.empty()) {
    const int32_t fd = *pending.begin();
    pending.erase(pending.begin());
    if (slots_of.count(fd)) continue;
    std::vector<int32_t> slots(r.maps[fd].max_entries);
    if (!slots.empty() &&
        hipMemcpy(slots.data(), (const void *)r.maps[fd].d.data, 4 * slots.size(), hipMemcpyDeviceToHost) != hipSuccess) {
      error = "prog array read failed";
      return -1;
    }
    slot_fds[fd] = slots;
    std::vector<int32_t> &ts = slots_of[fd];
    for (int32_t v : slots)
      if (v >= 0 && v < (int32_t)kMaxFds && r.kind[v] == HKind::PROG) {
        ts.push_back(v);
        if (!arrays_of_prog.count(v)) {
          const std::vector<uint8_t> &b = r.progs[v].insns;
          arrays_of((const RawInsn *)b.data(), b.size() / 8, arrays_of_prog[v]);
          for (int32_t a : arrays_of_prog[v]) pending.insert(a);
        }
      }
  }
  // Targets before the loaded program (which goes last behind a jump at
  // pc 0), callers before callees among them (reverse post-order): lane
  // groups run lowest pc first, so every target runs before the loaded
  // program's code it returns to -- lanes returning from different targets
  // (or failing the call) meet at the return point -- and a target that
  // other targets call runs after them, so the lanes that reach it from a
  // nested call join the lanes that called it directly (one group, one
  // pass over its code: tail-call line 1.30 -> 1.1x ms).  Lanes whose
  // nested call fails continue in their caller before the callee runs.
  std::vector<int32_t> order;
  std::set<int32_t> visited;
  std::function<void(int32_t)> visit = [&](int32_t t) {
    if (!visited.insert(t).second) return;
    for (int32_t a : arrays_of_prog[t])
      for (int32_t u : slots_of[a]) visit(u);
    order.push_back(t);
  };
  for (int32_t a : root_arrays)
    for (int32_t u : slots_of[a]) visit(u);
  std::reverse(order.begin(), order.end());
  std::vector<RawInsn> code;
  std::vector<uint32_t> entries;
  std::vector<int32_t> entry(kMaxFds, -1);
  uint32_t stack_need = base_stack;  // the deepest program of the image
  if (!order.empty()) code.push_back(RawInsn{});  // pc 0: ja to the loaded program
  for (int32_t t : order) {
    const std::vector<uint8_t> &bytes = r.progs[t].insns;
    const size_t n = bytes.size() / 8;
    if (code.size() + n + raw.size() + 1 > kMaxInsts || code.size() + n > 0x7fff) {
      link_note += "prog " + std::to_string(t) + ": image would exceed " + std::to_string(kMaxInsts) + " insns; ";
      continue;
    }
    LoadOut alone;
    std::string err;
    if (load_program((const RawInsn *)bytes.data(), n, hm, names, lddw, alone, err) < 0) {
      link_note += "prog " + std::to_string(t) + ": " + err + "; ";
      continue;
    }
    stack_need = std::max(stack_need, alone.big_stack ? kStackSize + 1 : alone.stack_size);
    entry[t] = (int32_t)code.size();
    entries.push_back((uint32_t)code.size());
    const RawInsn *c = (const RawInsn *)bytes.data();
    for (size_t i = 0; i < n; i++) {
      RawInsn x = c[i];
      if (x.code == 0x95) {  // exit -> return to the caller's frame
        x = RawInsn{};
        x.code = 0x85;
        x.imm = kRetHelper;
      }
      code.push_back(x);
      if (c[i].code == 0x18 && i + 1 < n) code.push_back(c[++i]);
    }
  }
  if (entries.empty()) {
    code.clear();  // nothing linked: the program alone
  } else {
    code[0].code = 0x05;  // ja +off
    code[0].off = (int16_t)(code.size() - 1);
  }
  code.insert(code.end(), raw.begin(), raw.end());
  if (!entries.empty()) {
    RawInsn ex{};
    ex.code = 0x95;
    code.push_back(ex);
  }
  LoadOut out;
  std::string err;
  if (load_program(code.data(), code.size(), hm, names, lddw, out, err, entries) < 0) {
    error = "tail-call image: " + err;
    return -1;
  }
  if (stack_need <= kLdsStackMax) {
    // every program's stack fits the LDS stack: the frames save that many bytes
    out.big_stack = false;
    out.stack_size = std::max<uint32_t>(8, stack_need);
  }
  auto im = std::make_shared<Image>();
  im->frame_words = (kFrameHdr + kFrameCtx + (out.big_stack ? kStackSize : out.stack_size)) / 8;
  im->gen = r.prog_gen;
  if (im->upload(std::move(out), error) < 0) return -1;
  // slot -> entry pc per reachable prog array (the image is relinked when
  // a prog, an array or a slot changes: Runtime::prog_gen)
  std::vector<int32_t> tslots(kMaxFds, -1);
  for (const auto &kv : slot_fds) {
    tslots[kv.first] = (int32_t)tslots.size();
    for (const int32_t v : kv.second)
      tslots.push_back(v >= 0 && v < (int32_t)kMaxFds && r.kind[v] == HKind::PROG ? entry[v] : -1);
  }
  if (hipMalloc((void **)&im->d_tail_entry, 4 * kMaxFds) != hipSuccess ||
      hipMemcpy(im->d_tail_entry, entry.data(), 4 * kMaxFds, hipMemcpyHostToDevice) != hipSuccess ||
      hipMalloc((void **)&im->d_tail_slots, 4 * tslots.size()) != hipSuccess ||
      hipMemcpy(im->d_tail_slots, tslots.data(), 4 * tslots.size(), hipMemcpyHostToDevice) != hipSuccess) {
    error = "device upload failed";
    return -1;
  }
  img = std::move(im);
  return 0;
}

}  // namespace bpftime_amd
