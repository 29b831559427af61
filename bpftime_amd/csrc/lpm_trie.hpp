// bpftime_amd: the host LPM trie (runtime/src/bpf_map/userspace/lpm_trie_map.cpp).
// The host keeps the authoritative trie (same node structure and update /
// logical-delete rules as the reference); the device holds a read-only
// replica (common.hpp DMap comment) uploaded before the next launch after a
// change (map_lpm.cpp).  Host-only: no device call in here.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <vector>

namespace bpftime_amd {

struct LpmTrie {
  struct Node {
    uint32_t plen = 0;
    bool inter = false;
    int32_t child[2] = {-1, -1};
    std::vector<uint8_t> data, value;
  };
  uint32_t dsz = 0, vsz = 0, max_entries = 0, cap = 0;
  std::vector<Node> nodes;
  int32_t root = -1;
  uint64_t entries = 0;

  // DIR-24-8 form of a trie with 4-byte keys (IPv4 routing), for device
  // lookups of full-length keys (prefixlen 32): t[a >> 8] for the top 24
  // address bits holds node + 1 of the node lookup() returns for every
  // address of that /24 (0: none), or 0x80000000 | g when the result
  // depends on the low byte, whose 256 results then sit in group g at
  // t[2^24 + 256 g].  Built by partitioning the address space the way the
  // walk does (lpm_trie_map.cpp:192-264, restated in lookup()): the
  // addresses reaching a node form one prefix block; those its prefix does
  // not match keep the result found above it, the matching ones continue to
  // its children, and a matching 32-bit node ends the walk (a deleted, i.e.
  // intermediate, one with no result: the reference's ENOENT, not the
  // covering prefix).  The blocks are disjoint and cover every address, so
  // each table entry is written by exactly one of them.  False when more
  // than max_groups /24s need a group.
  bool flat(std::vector<uint32_t> &t, uint32_t max_groups) const {
    t.assign(1u << 24, 0);
    uint32_t ng = 0;
    bool ok = true;
    auto top = [](uint32_t a, uint32_t len) { return len ? a & (~0u << (32 - len)) : 0u; };
    auto paint = [&](uint32_t a, uint32_t len, uint32_t v) {
      a = top(a, len);
      if (len <= 24) {
        const uint32_t j = a >> 8;
        std::fill(t.begin() + j, t.begin() + j + (1u << (24 - len)), v);
        return;
      }
      const uint32_t j = a >> 8;
      if (!(t[j] & 0x80000000u)) {
        if (ng >= max_groups) {
          ok = false;
          return;
        }
        t.resize(t.size() + 256, 0);
        t[j] = 0x80000000u | ng++;
      }
      const uint64_t g = (1u << 24) + 256ull * (t[j] & 0x7fffffffu) + (a & 0xff);
      std::fill(t.begin() + g, t.begin() + g + (1u << (32 - len)), v);
    };
    // (node, arrival block (a, len), result found above it)
    std::function<void(int32_t, uint32_t, uint32_t, uint32_t)> visit = [&](int32_t ni, uint32_t a, uint32_t len,
                                                                           uint32_t f) {
      if (!ok) return;
      if (ni < 0) {
        paint(a, len, f);
        return;
      }
      const Node &n = nodes[ni];
      const uint32_t np = n.plen;
      const uint32_t nd = top(((uint32_t)n.data[0] << 24) | ((uint32_t)n.data[1] << 16) |
                                  ((uint32_t)n.data[2] << 8) | n.data[3], np);
      const uint32_t c = std::min(len, np);
      if (top(a, c) != top(nd, c)) {  // no address of the block matches the node
        paint(a, len, f);
        return;
      }
      for (uint32_t i = len; i < np; i++)  // first mismatch at bit i
        paint(top(nd, i) | ((~nd) & (0x80000000u >> i)), i + 1, f);
      const uint32_t ml = std::max(len, np);
      const uint32_t m = len > np ? a : (top(a, len) | nd);  // the matching block (m, ml)
      if (np == 32) {
        paint(m, 32, n.inter ? 0 : (uint32_t)ni + 1);
        return;
      }
      const uint32_t f2 = n.inter ? f : (uint32_t)ni + 1;
      for (uint32_t b = 0; b < 2; b++) {
        const uint32_t bitv = b ? (0x80000000u >> np) : 0;
        if (ml > np && (m & (0x80000000u >> np)) != bitv) continue;
        const uint32_t nl = std::max(ml, np + 1);
        visit(n.child[b], top(top(m, np) | bitv | (m & ~top(~0u, np + 1)), nl), nl, f2);
      }
    };
    visit(root, 0, 0, 0);
    return ok;
  }

  int bit(const uint8_t *d, size_t i) const {  // :88-98
    if (i >= (size_t)dsz * 8) return 0;
    return (d[i / 8] >> (7 - (i % 8))) & 1;
  }
  size_t match(const Node &n, const uint8_t *key) const {  // :101-113
    uint32_t kp;
    memcpy(&kp, key, 4);
    const uint32_t lim = std::min(n.plen, kp);
    size_t i = 0;
    while (i < lim && bit(n.data.data(), i) == bit(key + 4, i)) i++;
    return i;
  }
  int32_t make(const uint8_t *key, uint32_t plen, const void *value, bool inter) {
    if (nodes.size() >= cap) return -1;
    Node n;
    n.plen = plen;
    n.inter = inter;
    n.data.assign(key + 4, key + 4 + dsz);
    n.value.assign(vsz, 0);
    if (!inter && value) memcpy(n.value.data(), value, vsz);
    nodes.push_back(std::move(n));
    return (int32_t)nodes.size() - 1;
  }
  const Node *lookup(const uint8_t *key) const {  // :192-264
    uint32_t kp;
    memcpy(&kp, key, 4);
    const uint32_t maxp = dsz * 8;
    if (kp > maxp) {
      errno = EINVAL;
      return nullptr;
    }
    int32_t node = root;
    const Node *found = nullptr;
    while (node >= 0) {
      const Node &n = nodes[node];
      const size_t ml = match(n, key);
      if (ml == maxp) {
        found = &n;
        break;
      }
      if (ml < n.plen) break;
      if (!n.inter) found = &n;
      if (ml < kp)
        node = n.child[bit(key + 4, n.plen)];
      else
        break;
    }
    if (!found || found->inter) {
      errno = ENOENT;
      return nullptr;
    }
    return found;
  }
  long update(const uint8_t *key, const void *value, uint64_t flags) {  // :266-488
    if (flags != 0 && flags != 1 && flags != 2) {
      errno = EINVAL;
      return -1;
    }
    uint32_t kp;
    memcpy(&kp, key, 4);
    const uint32_t maxp = dsz * 8;
    if (kp > maxp) {
      errno = EINVAL;
      return -1;
    }
    auto need_room = [&]() {
      if (flags == 2) {
        errno = ENOENT;
        return false;
      }
      if (entries >= max_entries) {
        errno = ENOSPC;
        return false;
      }
      if (nodes.size() + 2 > cap) {  // node pool of the device replica
        errno = ENOMEM;
        return false;
      }
      return true;
    };
    if (root < 0) {
      if (!need_room()) return -1;
      root = make(key, kp, value, false);
      entries++;
      return 0;
    }
    int32_t parent = -1, pbit = 0, node = -1;
    int32_t cur = root;
    size_t ml = 0;
    while (cur >= 0) {
      node = cur;
      const Node &n = nodes[cur];
      ml = match(n, key);
      if (n.plen != ml || n.plen == kp || n.plen == maxp) break;
      parent = cur;
      pbit = bit(key + 4, n.plen);
      cur = n.child[pbit];
    }
    auto set_slot = [&](int32_t v) {
      if (parent < 0)
        root = v;
      else
        nodes[parent].child[pbit] = v;
    };
    auto split = [&](int32_t at) {  // intermediate node at the split point
      const int32_t nn = make(key, kp, value, false);
      const int32_t im = make(key, (uint32_t)ml, nullptr, true);
      if (bit(key + 4, ml)) {
        nodes[im].child[0] = at;
        nodes[im].child[1] = nn;
      } else {
        nodes[im].child[0] = nn;
        nodes[im].child[1] = at;
      }
      set_slot(im);
      entries++;
      return 0L;
    };
    if (cur >= 0 && nodes[cur].plen == kp) {  // case 1
      if (match(nodes[cur], key) == kp) {
        Node &n = nodes[cur];
        if (flags == 1) {
          errno = EEXIST;
          return -1;
        }
        if (flags == 2 && n.inter) {
          errno = ENOENT;
          return -1;
        }
        if (n.inter) {
          if (entries >= max_entries) {
            errno = ENOSPC;
            return -1;
          }
          n.inter = false;
          entries++;
        }
        memcpy(n.value.data(), value, vsz);
        return 0;
      }
      if (!need_room()) return -1;
      return split(cur);
    }
    if (cur < 0) {  // case 2
      if (!need_room()) return -1;
      set_slot(make(key, kp, value, false));
      entries++;
      return 0;
    }
    (void)node;
    if (ml == kp) {  // case 3: the new prefix becomes cur's parent
      if (!need_room()) return -1;
      const int32_t nn = make(key, kp, value, false);
      nodes[nn].child[bit(nodes[cur].data.data(), ml)] = cur;
      set_slot(nn);
      entries++;
      return 0;
    }
    if (!need_room()) return -1;  // case 4
    return split(cur);
  }
  long remove(const uint8_t *key) {  // :490-541: logical deletion
    uint32_t kp;
    memcpy(&kp, key, 4);
    if (kp > dsz * 8) {
      errno = EINVAL;
      return -1;
    }
    int32_t cur = root, last = -1;
    while (cur >= 0) {
      last = cur;
      const Node &n = nodes[cur];
      const size_t ml = match(n, key);
      if (n.plen != ml || n.plen == kp) break;
      cur = n.child[bit(key + 4, n.plen)];
      last = cur;
    }
    if (last < 0 || nodes[last].plen != kp || match(nodes[last], key) != kp || nodes[last].inter) {
      errno = ENOENT;
      return -1;
    }
    nodes[last].inter = true;
    std::fill(nodes[last].value.begin(), nodes[last].value.end(), 0);
    if (entries) entries--;
    return 0;
  }
  int first_key(uint8_t *next) const {  // :543-590 (only the first key is implemented there)
    int32_t cur = root;
    while (cur >= 0) {
      const Node &n = nodes[cur];
      if (!n.inter) {
        memcpy(next, &n.plen, 4);
        memcpy(next + 4, n.data.data(), dsz);
        return 0;
      }
      cur = n.child[0] >= 0 ? n.child[0] : n.child[1];
    }
    errno = ENOENT;
    return -1;
  }
  // device replica image (common.hpp DMap comment): header {i32 root,
  // u32 nodes, u32 entries, u32 cap}, then the nodes in pool order
  void image(std::vector<uint8_t> &out, uint32_t slot, uint32_t key_off, uint32_t val_off) const {
    out.assign(16 + (size_t)nodes.size() * slot, 0);
    const uint32_t nn = (uint32_t)nodes.size(), ne = (uint32_t)entries;
    memcpy(out.data(), &root, 4);
    memcpy(out.data() + 4, &nn, 4);
    memcpy(out.data() + 8, &ne, 4);
    memcpy(out.data() + 12, &cap, 4);
    for (size_t i = 0; i < nodes.size(); i++) {
      uint8_t *b = out.data() + 16 + i * slot;
      const Node &n = nodes[i];
      const uint32_t inter = n.inter ? 1 : 0;
      memcpy(b, &n.plen, 4);
      memcpy(b + 4, &inter, 4);
      memcpy(b + 8, n.child, 8);
      memcpy(b + key_off, n.data.data(), dsz);
      memcpy(b + val_off, n.value.data(), vsz);
    }
  }
  // the inverse of image(): the trie an ORDERED batch left in the replica
  // (dev_helpers.hpp lpm_update / lpm_remove append nodes in pool order)
  bool from_image(const uint8_t *img, size_t bytes, uint32_t slot, uint32_t key_off, uint32_t val_off) {
    if (bytes < 16) return false;
    int32_t rt_;
    uint32_t nn, ne;
    memcpy(&rt_, img, 4);
    memcpy(&nn, img + 4, 4);
    memcpy(&ne, img + 8, 4);
    if (nn > cap || 16 + (size_t)nn * slot > bytes || rt_ >= (int32_t)nn) return false;
    nodes.assign(nn, Node{});
    for (uint32_t i = 0; i < nn; i++) {
      const uint8_t *b = img + 16 + (size_t)i * slot;
      Node &n = nodes[i];
      uint32_t inter;
      memcpy(&n.plen, b, 4);
      memcpy(&inter, b + 4, 4);
      n.inter = inter != 0;
      memcpy(n.child, b + 8, 8);
      n.data.assign(b + key_off, b + key_off + dsz);
      n.value.assign(b + val_off, b + val_off + vsz);
    }
    root = rt_;
    entries = ne;
    return true;
  }
};

}  // namespace bpftime_amd
