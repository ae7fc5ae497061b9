// Score plans: which score columns an utterance's graph needs, in the order the scoring kernels walk them, and the graph
// depths that tell a window's band of columns (include/mfa_hip.h).  Pure host graph analysis — breadth-first depths, the
// smallest depth still reachable from a state (Tarjan's strongly connected components), column clustering and ordering;
// nothing here touches the device.
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/mfa_hip.h"

extern "C" {

MFA_API int mfa_fst_first_frames(int32_t n_states, const int32_t *h_arc_off, const int32_t *h_arc_next, int32_t start,
                                 int32_t *h_depth) {
  if (n_states <= 0 || start < 0 || start >= n_states) return -1;
  for (int s = 0; s < n_states; s++) h_depth[s] = INT32_MAX;
  std::vector<int32_t> queue;
  queue.reserve(n_states);
  queue.push_back(start);
  h_depth[start] = 0;
  for (size_t q = 0; q < queue.size(); q++) {  // breadth-first: unit arc lengths
    const int s = queue[q];
    for (int a = h_arc_off[s]; a < h_arc_off[s + 1]; a++) {
      const int d = h_arc_next[a];
      if (d < 0 || d >= n_states) return -1;
      if (h_depth[d] == INT32_MAX) { h_depth[d] = h_depth[s] + 1; queue.push_back(d); }
    }
  }
  return 0;
}

// The same with epsilon input arcs (h_arc_pdf[a] < 0) counting for nothing: depth = fewest EMITTING arcs from the start state —
// the first frame a token can sit on the state, FasterDecoder's ProcessNonemitting moving tokens along epsilon arcs within a
// frame.  0-1 breadth-first search.
static int fst_first_frames_eps(int32_t n_states, const int32_t *h_arc_off, const int32_t *h_arc_next, const int32_t *h_arc_pdf,
                                int32_t start, int32_t *h_depth) {
  if (n_states <= 0 || start < 0 || start >= n_states) return -1;
  for (int s = 0; s < n_states; s++) h_depth[s] = INT32_MAX;
  std::vector<int32_t> cur, nxt;
  cur.push_back(start);
  h_depth[start] = 0;
  int32_t level = 0;
  while (!cur.empty()) {
    for (size_t q = 0; q < cur.size(); q++) {            // (cur grows while epsilon arcs are followed)
      const int s = cur[q];
      if (h_depth[s] != level) continue;                 // reached more cheaply in the meantime
      for (int a = h_arc_off[s]; a < h_arc_off[s + 1]; a++) {
        const int d = h_arc_next[a];
        if (d < 0 || d >= n_states) return -1;
        const int32_t nd = level + (h_arc_pdf[a] < 0 ? 0 : 1);
        if (nd < h_depth[d]) { h_depth[d] = nd; (nd == level ? cur : nxt).push_back(d); }
      }
    }
    cur.swap(nxt); nxt.clear();
    level++;
  }
  return 0;
}

MFA_API int mfa_fst_last_depths(int32_t n_states, const int32_t *h_arc_off, const int32_t *h_arc_next, int32_t start,
                                const int32_t *h_bfs_depth, int32_t *h_depth) {
  if (n_states <= 0 || start < 0 || start >= n_states) return -1;
  for (int a = 0; a < h_arc_off[n_states]; a++)
    if (h_arc_next[a] < 0 || h_arc_next[a] >= n_states) return -1;
  // h_depth[s] = the smallest BFS depth among the states reachable from s (s included).  Computed over the graph's
  // condensation: strongly connected components (self-loops, the small cycles of an ergodic silence topology) come out of
  // Tarjan's algorithm (iterative) in reverse topological order, i.e. sinks first — exactly the order this needs.
  std::vector<int32_t> index(n_states, -1), low(n_states, 0), comp(n_states, -1), stack, next_arc(n_states, 0);
  std::vector<char> on_stack(n_states, 0);
  std::vector<int32_t> call;   // DFS stack of states
  int32_t counter = 0, n_comp = 0;
  call.push_back(start);
  index[start] = low[start] = counter++;
  stack.push_back(start); on_stack[start] = 1;
  next_arc[start] = h_arc_off[start];
  std::vector<int32_t> comp_first;   // members of component k: comp_members[comp_first[k] .. comp_first[k+1])
  std::vector<int32_t> comp_members;
  while (!call.empty()) {
    const int s = call.back();
    if (next_arc[s] < h_arc_off[s + 1]) {
      const int d = h_arc_next[next_arc[s]++];
      if (index[d] < 0) {
        index[d] = low[d] = counter++;
        stack.push_back(d); on_stack[d] = 1;
        next_arc[d] = h_arc_off[d];
        call.push_back(d);
      } else if (on_stack[d]) {
        low[s] = std::min(low[s], index[d]);
      }
    } else {
      call.pop_back();
      if (!call.empty()) low[call.back()] = std::min(low[call.back()], low[s]);
      if (low[s] == index[s]) {
        comp_first.push_back((int32_t)comp_members.size());
        for (;;) {
          const int v = stack.back(); stack.pop_back(); on_stack[v] = 0;
          comp[v] = n_comp;
          comp_members.push_back(v);
          if (v == s) break;
        }
        n_comp++;
      }
    }
  }
  comp_first.push_back((int32_t)comp_members.size());
  // an arc s -> d between different components has comp[d] < comp[s]: ascending component order visits successors first
  std::vector<int32_t> cmin(n_comp, INT32_MAX);
  bool cyclic = false;
  for (int k = 0; k < n_comp; k++) {
    if (comp_first[k + 1] - comp_first[k] > 1) cyclic = true;
    int32_t m = INT32_MAX;
    for (int i = comp_first[k]; i < comp_first[k + 1]; i++) {
      const int s = comp_members[i];
      m = std::min(m, h_bfs_depth[s]);
      for (int a = h_arc_off[s]; a < h_arc_off[s + 1]; a++) {
        const int cd = comp[h_arc_next[a]];
        if (cd != k) m = std::min(m, cmin[cd]);
      }
    }
    cmin[k] = m;
  }
  for (int s = 0; s < n_states; s++) h_depth[s] = comp[s] >= 0 ? cmin[comp[s]] : 0;
  return cyclic ? 1 : 0;
}

// Score columns of one utterance for mfa_align_features_batch / mfa_gmm_score_batch — see include/mfa_hip.h.
MFA_API int mfa_build_score_plan(int32_t n_states, const int32_t *h_arc_off, const int32_t *h_arc_next,
                                 const int32_t *h_arc_pdf, int32_t start, int32_t num_pdfs, const int32_t *h_pdf_class,
                                 int32_t cluster_span, int32_t *h_state_depth, int32_t *h_arc_col, int32_t *h_col_pdf,
                                 int32_t *h_col_first, int32_t *h_col_last, int32_t *h_class_counts, int32_t *h_n_cols) {
  return mfa_build_score_plan_grouped(n_states, h_arc_off, h_arc_next, h_arc_pdf, start, num_pdfs, h_pdf_class, cluster_span,
                                      1, h_state_depth, h_arc_col, h_col_pdf, h_col_first, h_col_last, h_class_counts, nullptr,
                                      h_n_cols);
}

MFA_API int mfa_build_score_plans_batch(int32_t n_utt, const int64_t *h_state_off, const int64_t *h_arc_base,
                                        const int32_t *h_arc_off, const int32_t *h_arc_next, const int32_t *h_arc_pdf,
                                        const int32_t *h_start, int32_t num_pdfs, const int32_t *h_pdf_class,
                                        int32_t cluster_span, int32_t groups, int32_t n_threads, int32_t *h_state_depth,
                                        int32_t *h_arc_col, int32_t *h_col_pdf, int32_t *h_col_first, int32_t *h_col_last,
                                        int32_t *h_class_counts, int32_t *h_group_counts, int32_t *h_n_cols,
                                        int32_t *h_bad_utt) {
  if (n_utt < 0) return -1;
  std::atomic<int> next(0), first_bad(INT32_MAX);
  std::vector<int> codes((size_t)std::max(n_utt, 1), 0);
  auto work = [&]() {
    for (;;) {
      const int u = next.fetch_add(1);
      if (u >= n_utt) break;
      const int64_t s0 = h_state_off[u], a0 = h_arc_base[u];
      const int32_t ns = (int32_t)(h_state_off[u + 1] - s0);
      const int rc = mfa_build_score_plan_grouped(ns, h_arc_off + s0 + u, h_arc_next + a0, h_arc_pdf + a0, h_start[u], num_pdfs,
                                                  h_pdf_class, cluster_span, groups, h_state_depth + 2 * s0, h_arc_col + a0,
                                                  h_col_pdf + a0, h_col_first + a0, h_col_last + a0, h_class_counts + 6 * (size_t)u,
                                                  groups > 1 ? h_group_counts + (size_t)groups * u : nullptr, h_n_cols + u);
      codes[u] = rc;
      if (rc != 0) { int cur = first_bad.load(); while (u < cur && !first_bad.compare_exchange_weak(cur, u)) {} }
    }
  };
  const int nt = std::max(1, std::min(n_threads, n_utt));
  if (nt == 1) work();
  else {
    std::vector<std::thread> ts;
    for (int t = 0; t < nt; t++) ts.emplace_back(work);
    for (auto &t : ts) t.join();
  }
  const int bad = first_bad.load();
  if (bad != INT32_MAX) { if (h_bad_utt) *h_bad_utt = bad; return codes[bad]; }
  return 0;
}

MFA_API int mfa_build_score_plan_grouped(int32_t n_states, const int32_t *h_arc_off, const int32_t *h_arc_next,
                                         const int32_t *h_arc_pdf, int32_t start, int32_t num_pdfs, const int32_t *h_pdf_class,
                                         int32_t cluster_span, int32_t groups, int32_t *h_state_depth, int32_t *h_arc_col,
                                         int32_t *h_col_pdf, int32_t *h_col_first, int32_t *h_col_last, int32_t *h_class_counts,
                                         int32_t *h_group_counts, int32_t *h_n_cols) {
  if (groups < 1 || groups > MFA_PLAN_MAX_GROUPS || (groups > 1 && !h_group_counts)) return -3;
  if (n_states <= 0 || start < 0 || start >= n_states) return -1;
  const int n_arcs = h_arc_off[n_states];
  std::vector<int32_t> bfs(n_states), low(n_states);
  bool has_eps = false;
  for (int a = 0; a < n_arcs; a++) if (h_arc_pdf[a] < 0) { has_eps = true; break; }
  // (an arc with pdf -1 is an epsilon input arc: no score column, no frame consumed)
  if ((has_eps ? fst_first_frames_eps(n_states, h_arc_off, h_arc_next, h_arc_pdf, start, bfs.data())
               : mfa_fst_first_frames(n_states, h_arc_off, h_arc_next, start, bfs.data())) != 0) return -1;
  if (mfa_fst_last_depths(n_states, h_arc_off, h_arc_next, start, bfs.data(), low.data()) < 0) return -1;
  for (int s = 0; s < n_states; s++) {
    h_state_depth[2 * s] = bfs[s] == INT32_MAX ? 0 : bfs[s];
    h_state_depth[2 * s + 1] = bfs[s] == INT32_MAX ? 0 : low[s];
  }
  // arcs by (pdf, BFS depth of the source state); a column = a run of one pdf's arcs whose depths stay within
  // cluster_span of the run's first (cluster_span <= 0: one column per pdf)
  std::vector<int32_t> src(n_arcs), order(n_arcs);
  for (int s = 0; s < n_states; s++)
    for (int a = h_arc_off[s]; a < h_arc_off[s + 1]; a++) src[a] = s;
  order.clear();
  for (int a = 0; a < n_arcs; a++) {
    if (h_arc_pdf[a] == -1) continue;                    // epsilon input arc
    if (h_arc_pdf[a] < 0 || h_arc_pdf[a] >= num_pdfs) return -2;
    if (h_pdf_class[h_arc_pdf[a]] < 0 || h_pdf_class[h_arc_pdf[a]] > 5) return -2;
    order.push_back(a);
  }
  const int n_emit = (int)order.size();
  std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
    if (h_arc_pdf[x] != h_arc_pdf[y]) return h_arc_pdf[x] < h_arc_pdf[y];
    return bfs[src[x]] < bfs[src[y]];
  });
  struct Col { int32_t pdf, first, last, cls; };
  std::vector<Col> cols;
  std::vector<int32_t> col_of_arc(n_arcs, -1);
  for (int i = 0; i < n_emit; i++) {
    const int a = order[i], pdf = h_arc_pdf[a], d = bfs[src[a]];
    const bool fresh = cols.empty() || cols.back().pdf != pdf ||
                       (cluster_span > 0 && ((int64_t)d - cols.back().first > cluster_span));
    if (fresh) cols.push_back({pdf, d, d, h_pdf_class[pdf]});
    cols.back().last = std::max(cols.back().last, d);
    col_of_arc[a] = (int32_t)cols.size() - 1;
  }
  // kernel order: slot class, (class 0 only: pdf id mod `groups` — the XCD whose L2 keeps that part of the model), then
  // ascending first depth (ties: pdf id, then depth — the creation order)
  const int n_cols = (int)cols.size();
  std::vector<int32_t> perm(n_cols), rank(n_cols);
  for (int i = 0; i < n_cols; i++) perm[i] = i;
  auto group_of = [&](const Col &c) { return c.cls == 0 ? c.pdf % groups : 0; };
  std::stable_sort(perm.begin(), perm.end(), [&](int32_t x, int32_t y) {
    if (cols[x].cls != cols[y].cls) return cols[x].cls < cols[y].cls;
    const int gx = group_of(cols[x]), gy = group_of(cols[y]);
    if (gx != gy) return gx < gy;
    return cols[x].first < cols[y].first;
  });
  for (int k = 0; k < 6; k++) h_class_counts[k] = 0;
  if (h_group_counts) for (int k = 0; k < groups; k++) h_group_counts[k] = 0;
  int32_t run_cls = -1, run_grp = -1, run_max = 0;
  for (int i = 0; i < n_cols; i++) {
    const Col &cl = cols[perm[i]];
    const int grp = group_of(cl);
    rank[perm[i]] = i;
    h_col_pdf[i] = cl.pdf;
    h_col_first[i] = cl.first;
    if (cl.cls != run_cls || grp != run_grp) { run_cls = cl.cls; run_grp = grp; run_max = cl.last; }
    run_max = std::max(run_max, cl.last);
    h_col_last[i] = run_max;            // running max inside the class (class 0: inside the group): non-decreasing along it
    h_class_counts[cl.cls]++;
    if (h_group_counts && cl.cls == 0) h_group_counts[grp]++;
  }
  for (int a = 0; a < n_arcs; a++) h_arc_col[a] = col_of_arc[a] >= 0 ? rank[col_of_arc[a]] : 0;
  *h_n_cols = n_cols;
  return 0;
}

}  // extern "C"
