// The geometry threads: a scene's chain of strided grids and the views behind them, built beside the feature pass.
#include <condition_variable>
#include <string>
#include <thread>

#include "grid_internal.h"

namespace d3d {

// The chain of strided grids of one scene, run by a thread of its own (d3d_geometry_async_start): every new grid costs
// one blocking read-back of its site count, and a caller that builds the chain itself cannot enqueue feature kernels
// while it waits.  The thread builds the listed rulebooks in order on the geometry stream and publishes, per entry,
// the output site count and an event; the caller picks an entry up when it needs it (d3d_geometry_async_wait).
// A new strided grid is complete (hash table, coordinates, site count) as soon as its count has been read back, before
// the strided rulebook built with it: run_grid_chain enters it into the metadata then.
struct GeoAsync {
  std::thread th, th_views;                 // the grids (blocking read-backs) / the views behind them; started with the
  bool threads_up = false, stop = false;    // first chain of this metadata and kept (a handle serves scene after scene)
  int job = 0, job_done[2] = {0, 0};        // chains started / finished by each worker
  std::mutex mu;
  std::condition_variable cv;
  std::vector<std::array<int, 13>> specs;   // kind, in_size, out_size, filter, stride
  std::vector<int> n_out;
  std::vector<hipEvent_t> ev, gev;          // pools, reused from scene to scene: entry done / its grid complete
  std::vector<char> ready, grid_ready;      // entry built (grids) / enqueued (views); grid of a kind-1 entry complete
  int rc = 0, device = 0;
  std::string err;
  hipStream_t stream = nullptr, view_stream = nullptr;
};
// publishes the outcome of entry i; returns false when the chain has failed (here or in the other worker)
static bool geo_publish(GeoAsync *g, int i, int rc, int n_out) {
  std::lock_guard<std::mutex> lk(g->mu);
  if (rc == D3D_OK) {
    g->n_out[i] = n_out;
    g->ready[i] = 1;
  } else if (g->rc == D3D_OK) {
    g->rc = rc;
    g->err = d3d_last_error();
  }
  g->cv.notify_all();
  return g->rc == D3D_OK;
}
static int geo_begin(GeoAsync *g) {
  if (hipSetDevice(g->device) == hipSuccess) return D3D_OK;
  set_error("geometry thread: hipSetDevice(%d) failed", g->device);
  return D3D_ERR_HIP;
}

// levels of the first chain: the feature pass wants the first strided grid (and its rulebooks) a few hundred microseconds
// after the input grid, before a chain over all levels has finished -- so it gets a read-back of its own
constexpr size_t kChainHead = 1;

static void geo_run_grids(d3d_meta *m, GeoAsync *g) {      // the grids of the pyramid: two chains, two read-backs
  int rc = geo_begin(g);
  const int n = (int)g->specs.size();
  std::vector<int> rows;
  for (int i = 0; i < n; i++)
    if (g->specs[i][0] == 1 || g->specs[i][0] == 3) rows.push_back(i);
  if (rows.empty()) return;
  struct Hook {
    GeoAsync *g;
    const std::vector<int> *rows;
    bool failed;
    int first;                              // row of `rows` the running chain's level 0 is
  } hk = {g, &rows, false, 0};
  std::vector<ChainSpec> specs(rows.size());
  for (size_t j = 0; j < rows.size(); j++) {
    const int *sp = g->specs[rows[j]].data() + 1;
    for (int d = 0; d < 3; d++) {
      specs[j].in_size[d] = sp[d];
      specs[j].out_size[d] = sp[3 + d];
      specs[j].filt[d] = sp[6 + d];
      specs[j].stride[d] = sp[9 + d];
    }
    specs[j].need_dec = g->specs[rows[j]][0] == 1;      // kind 3: a strided grid whose decoded table nobody will ask for
  }
  const ChainHook on_grid = [](void *a, int level, int, hipStream_t on) {       // the grid exists: its views may start
    Hook *h = (Hook *)a;
    const int i = (*h->rows)[h->first + level];
    if (hipEventRecord(h->g->gev[i], on) != hipSuccess) return;
    std::lock_guard<std::mutex> lk(h->g->mu);
    h->g->grid_ready[i] = 1;
    h->g->cv.notify_all();
  };
  const ChainHook on_done = [](void *a, int level, int n_sites, hipStream_t on) {   // its strided rulebook is enqueued
    Hook *h = (Hook *)a;
    const int i = (*h->rows)[h->first + level];
    int rc2 = D3D_OK;
    if (hipEventRecord(h->g->ev[i], on) != hipSuccess) {
      set_error("geometry thread: hipEventRecord failed");
      rc2 = D3D_ERR_HIP;
    }
    if (!geo_publish(h->g, i, rc2, n_sites)) h->failed = true;
  };
  const size_t cut = std::min(kChainHead, specs.size());
  for (int part = 0; part < 2 && rc == D3D_OK && !hk.failed; part++) {
    const size_t lo = part == 0 ? 0 : cut, hi = part == 0 ? cut : specs.size();
    if (lo >= hi) continue;
    std::vector<ChainSpec> seg(specs.begin() + lo, specs.begin() + hi);
    std::vector<int> n_out;
    hk.first = (int)lo;
    rc = run_grid_chain(m, seg, g->stream, n_out, on_grid, on_done, &hk);
  }
  if (rc != D3D_OK) geo_publish(g, rows[0], rc, 0);
}
static void geo_run_views(d3d_meta *m, GeoAsync *g) {      // the views: each behind the newest grid listed before it
  int rc = geo_begin(g);
  const int n = (int)g->specs.size();
  int dep = -1;
  for (int i = 0; i < n; i++) {
    const int kind = g->specs[i][0];
    if (kind == 1 || kind == 3) {
      dep = i;
      continue;
    }
    // a submanifold view needs the grid only; a deconvolution view the strided rulebook built with it
    bool early = false;
    if (dep >= 0) {
      std::unique_lock<std::mutex> lk(g->mu);
      g->cv.wait(lk, [&] { return g->ready[dep] || (kind == 0 && g->grid_ready[dep]) || g->rc != D3D_OK; });
      if (!g->ready[dep] && !(kind == 0 && g->grid_ready[dep])) return;
      early = !g->ready[dep];
    }
    const int *sp = g->specs[i].data() + 1;
    hipStream_t on = g->view_stream;
    if (rc == D3D_OK && dep >= 0 && hipStreamWaitEvent(on, early ? g->gev[dep] : g->ev[dep], 0) != hipSuccess) {
      set_error("geometry thread: hipStreamWaitEvent failed");
      rc = D3D_ERR_HIP;
    }
    if (rc == D3D_OK)
      rc = kind == 0 ? d3d_subm_prepare(m, sp, sp + 6, on, nullptr)
                     : d3d_deconv_prepare(m, sp, sp + 3, sp + 6, sp + 9, on, nullptr);
    if (rc == D3D_OK && hipEventRecord(g->ev[i], on) != hipSuccess) {
      set_error("geometry thread: hipEventRecord failed");
      rc = D3D_ERR_HIP;
    }
    if (!geo_publish(g, i, rc, 0)) return;
  }
}

static void geo_worker(d3d_meta *m, GeoAsync *g, int which) {
  int seen = 0;
  for (;;) {
    {
      std::unique_lock<std::mutex> lk(g->mu);
      g->cv.wait(lk, [&] { return g->stop || g->job != seen; });
      if (g->stop) return;
      seen = g->job;
    }
    if (which == 0) geo_run_grids(m, g);
    else geo_run_views(m, g);
    std::lock_guard<std::mutex> lk(g->mu);
    g->job_done[which] = seen;
    g->cv.notify_all();
  }
}
void geo_async_join(d3d_meta *m) {
  GeoAsync *g = (GeoAsync *)m->geo_async;
  if (!g || !g->threads_up) return;
  std::unique_lock<std::mutex> lk(g->mu);
  g->cv.wait(lk, [&] { return g->job_done[0] == g->job && g->job_done[1] == g->job; });
}
void geo_async_free(d3d_meta *m) {
  GeoAsync *g = (GeoAsync *)m->geo_async;
  if (!g) return;
  geo_async_join(m);
  if (g->threads_up) {
    {
      std::lock_guard<std::mutex> lk(g->mu);
      g->stop = true;
      g->cv.notify_all();
    }
    g->th.join();
    g->th_views.join();
  }
  for (hipEvent_t e : g->ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : g->gev) (void)hipEventDestroy(e);
  delete g;
  m->geo_async = nullptr;
}

}  // namespace d3d

using namespace d3d;

extern "C" {

int d3d_geometry_async_start(d3d_meta *m, const int *specs, int n, void *stream, void *view_stream) {
  D3D_REQUIRE(m && (n == 0 || specs) && n >= 0 && n <= 128, "geometry_async_start: bad arguments");
  D3D_REQUIRE(m->geo_locked && (hipStream_t)stream == m->geo_stream,
              "geometry_async_start: `stream` must be the metadata's geometry stream (d3d_meta_set_geometry_stream)");
  for (int i = 0; i < n; i++) {
    const int kind = specs[i * 13];
    D3D_REQUIRE(kind >= 0 && kind <= 3, "geometry_async_start: entry %d has kind %d (0 submanifold view, 1 strided grid, "
                "2 deconvolution view, 3 strided grid without a deconvolution view)", i, kind);
    D3D_REQUIRE(kind == 1 || kind == 3 || (view_stream && (hipStream_t)view_stream == m->plan_stream),
                "geometry_async_start: views need the metadata's plan stream (d3d_meta_set_plan_stream)");
  }
  geo_async_join(m);
  GeoAsync *g = (GeoAsync *)m->geo_async;
  if (!g) m->geo_async = g = new GeoAsync();
  g->specs.resize(n);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < 13; j++) g->specs[i][j] = specs[i * 13 + j];
  g->n_out.assign(n, 0);
  while ((int)g->ev.size() < n) {
    hipEvent_t e, e2;
    D3D_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    g->ev.push_back(e);
    D3D_HIP_CHECK(hipEventCreateWithFlags(&e2, hipEventDisableTiming));
    g->gev.push_back(e2);
  }
  {
    std::lock_guard<std::mutex> lk(g->mu);
    g->ready.assign(n, 0);
    g->grid_ready.assign(n, 0);
    g->rc = D3D_OK;
    g->err.clear();
    g->stream = (hipStream_t)stream;
    g->view_stream = (hipStream_t)view_stream;
  }
  D3D_HIP_CHECK(hipGetDevice(&g->device));
  if (!g->threads_up) {
    g->th = std::thread(geo_worker, m, g, 0);
    g->th_views = std::thread(geo_worker, m, g, 1);
    g->threads_up = true;
  }
  std::lock_guard<std::mutex> lk(g->mu);
  g->job++;
  g->cv.notify_all();
  return D3D_OK;
}

int d3d_geometry_async_wait(d3d_meta *m, int index, int *n_out_host, void *wait_stream) {
  D3D_REQUIRE(m && m->geo_async, "geometry_async_wait: no chain was started");
  GeoAsync *g = (GeoAsync *)m->geo_async;
  D3D_REQUIRE(index >= 0 && index < (int)g->specs.size(), "geometry_async_wait: entry %d of %d", index, (int)g->specs.size());
  {
    std::unique_lock<std::mutex> lk(g->mu);
    g->cv.wait(lk, [&] { return g->ready[index] || g->rc != D3D_OK; });
    if (!g->ready[index]) {
      set_error("geometry thread: %s", g->err.c_str());
      return g->rc;
    }
    if (n_out_host) *n_out_host = g->n_out[index];
  }
  D3D_HIP_CHECK(hipStreamWaitEvent((hipStream_t)wait_stream, g->ev[index], 0));
  return D3D_OK;
}

int d3d_geometry_async_finish(d3d_meta *m) {
  D3D_REQUIRE(m, "null metadata");
  geo_async_join(m);
  GeoAsync *g = (GeoAsync *)m->geo_async;
  if (g && g->rc != D3D_OK) {
    set_error("geometry thread: %s", g->err.c_str());
    return g->rc;
  }
  return D3D_OK;
}

}  // extern "C"
