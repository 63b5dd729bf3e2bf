// dvh_api.cpp -- C ABI of libdervet_hip (declared in include/dervet_hip.h): the handle's lifetime, options, setters
// and dvh_last_* getters, and the communicator wrappers.  The solves are in dvh_solve.cpp (tier drivers:
// dvh_cascade.cpp), the other entry points in dvh_api_build.cpp, dvh_api_outage.cpp, dvh_api_valuation.cpp,
// dvh_api_value_sizing.cpp and dvh_sizing.cpp.  The handle owns whatever any of them makes (dvh_handle.h): dvh_destroy
// selects the device, waits on the stream and deletes it.
#include "dvh_handle.h"

#define DVH_VERSION_STRING "dervet_hip 0.1.0 (gfx950, restarted reflected-Halpern PDHG)"

namespace dvh {
HandleView handle_view(dvh_handle* h) { return HandleView{h->device, h->stream, &h->opts, &h->err, &h->sizing.p}; }
}  // namespace dvh

extern "C" {

const char* dvh_version(void) { return DVH_VERSION_STRING; }

void dvh_default_options(dvh_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->eps = 1e-6;
  o->max_iters = 100000;
  o->check_every = 32;
  o->kkt_every = 4;
  o->ruiz_iters = 10;
  o->power_iters = 64;
  o->step_safety = 0.998;
  o->reflection = 1.0;
  o->restart_sufficient = 0.2;
  o->restart_necessary = 0.8;
  o->restart_artificial = 0.1;
  o->primal_weight_theta = 1.0;
  o->verbose = 0;
  o->eps_obj = 1e-6;
}

static std::string check_options(const dvh_options* o) {
  if (!(o->eps > 0.0)) return "eps must be > 0";
  if (!(o->eps_obj >= 0.0)) return "eps_obj must be >= 0";
  if (o->max_iters <= 0) return "max_iters must be > 0";
  if (o->check_every <= 0) return "check_every must be > 0";
  if (o->kkt_every <= 0) return "kkt_every must be > 0";
  if (o->kkt_predict < 0) return "kkt_predict must be >= 0";
  if (o->certify < 0 || o->certify_iters < 0) return "certify and certify_iters must be >= 0";
  if (o->ruiz_iters < 0 || o->power_iters <= 0) return "ruiz_iters must be >= 0 and power_iters > 0";
  if (!(o->step_safety > 0.0 && o->step_safety < 1.0)) return "step_safety must be in (0, 1)";
  if (!(o->reflection >= 0.0 && o->reflection <= 1.0)) return "reflection must be in [0, 1]";
  return "";
}

static int create_one(int dev, const dvh_options* opts, dvh_handle** out);

int dvh_create_devices(const int32_t* devices, int32_t n, const dvh_options* opts, dvh_handle** out) {
  if (!out || !devices || n < 1) return DVH_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return DVH_ERR_HIP;
  for (int i = 0; i < n; ++i)
    if (devices[i] < 0 || devices[i] >= ndev) return DVH_ERR_ARG;
  dvh_handle* h = nullptr;
  if (int rc = create_one(devices[0], opts, &h)) return rc;
  for (int i = 1; i < n; ++i) {
    dvh_handle* p = nullptr;
    if (int rc = create_one(devices[i], opts, &p)) {
      dvh_destroy(h);
      return rc;
    }
    h->peers.push_back(p);
  }
  *out = h;
  return DVH_OK;
}

int dvh_create(int device_mask, const dvh_options* opts, dvh_handle** out) {
  if (!out) return DVH_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return DVH_ERR_HIP;
  std::vector<int32_t> devs;
  for (int d = 0; d < 31 && d < ndev; ++d)
    if ((device_mask >> d) & 1) devs.push_back(d);
  if (device_mask <= 0) devs = {0};
  if (devs.empty() || (device_mask >> std::min(ndev, 31)) != 0) return DVH_ERR_ARG;  // a bit beyond the devices
  return dvh_create_devices(devs.data(), (int32_t)devs.size(), opts, out);
}

static int create_one(int dev, const dvh_options* opts, dvh_handle** out) {
  dvh_handle* h = new dvh_handle();
  h->device = dev;
  dvh_default_options(&h->opts);
  if (opts) {
    std::string m = check_options(opts);
    if (!m.empty()) {
      delete h;
      return DVH_ERR_ARG;
    }
    h->opts = *opts;
  }
  if (hipSetDevice(dev) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return DVH_ERR_HIP;
  }
  for (DevEvent& e : h->ev)
    if (e.ensure() != hipSuccess) {
      dvh_destroy(h);
      return DVH_ERR_HIP;
    }
  {  // Halpern weight table 1/(k+2): exact IEEE quotients, identical to the host restatement
    std::vector<double> tab(dvh::kHalpernTab);
    for (int k = 0; k < dvh::kHalpernTab; ++k) tab[k] = 1.0 / (k + 2.0);
    if (h->d_hinv.ensure(sizeof(double) * tab.size()) != hipSuccess ||
        hipMemcpy(h->d_hinv.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice) != hipSuccess) {
      dvh_destroy(h);
      return DVH_ERR_HIP;
    }
  }
  *out = h;
  return DVH_OK;
}

int dvh_set_options(dvh_handle* h, const dvh_options* opts) {
  if (!h || !opts) return DVH_ERR_ARG;
  std::string m = check_options(opts);
  if (!m.empty()) return fail(h, DVH_ERR_ARG, m);
  h->opts = *opts;
  for (dvh_handle* p : h->peers) p->opts = *opts;
  return DVH_OK;
}

int dvh_device_count(const dvh_handle* h) { return h ? 1 + (int)h->peers.size() : 0; }

int dvh_destroy(dvh_handle* h) {
  if (!h) return DVH_ERR_ARG;
  for (dvh_handle* p : h->peers) dvh_destroy(p);
  h->peers.clear();
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  delete h;  // pinned words, buffers, events, large / comm / sizing, the stream (dvh_handle.h)
  return DVH_OK;
}

const char* dvh_last_error(const dvh_handle* h) { return h ? h->err.c_str() : "null handle"; }

// ---- the result all-gather across ranks (dvh_comm.cpp)
int dvh_comm_unique_id(dvh_handle* h, uint8_t* id) {
  if (!h || !id) return DVH_ERR_ARG;
  return dvh::comm_unique_id(id, &h->err);
}

int dvh_comm_init(dvh_handle* h, int32_t rank, int32_t world, const uint8_t* id) {
  if (!h || !id || world < 1 || rank < 0 || rank >= world) return fail(h, DVH_ERR_ARG, "dvh_comm_init: rank / world");
  if (!h->peers.empty())
    return fail(h, DVH_ERR_ARG, "dvh_comm_init: one communicator rank per device; this handle spans several");
  if (h->comm) return fail(h, DVH_ERR_ARG, "dvh_comm_init: the handle already has a communicator");
  return dvh::comm_init(h->device, rank, world, id, &h->comm, &h->err);
}

int dvh_comm_info(const dvh_handle* h, int32_t* rank_world) {
  if (!h || !rank_world) return DVH_ERR_ARG;
  if (!h->comm) {
    rank_world[0] = 0;
    rank_world[1] = 0;
    return DVH_OK;
  }
  int r = 0, w = 0;
  dvh::comm_info(h->comm.get(), &r, &w);
  rank_world[0] = r;
  rank_world[1] = w;
  return DVH_OK;
}

int dvh_gather_results(dvh_handle* h, const void* rows, uint64_t bytes_per_rank, void* out, void* stream) {
  if (!h || !rows || !out) return DVH_ERR_ARG;
  if (!h->comm) return fail(h, DVH_ERR_ARG, "dvh_gather_results: no communicator (dvh_comm_init)");
  if (bytes_per_rank == 0) return DVH_OK;
  hipSetDevice(h->device);
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  return dvh::comm_all_gather(h->comm.get(), rows, out, (size_t)bytes_per_rank, s, &h->err);
}
const char* dvh_last_warning(const dvh_handle* h) { return h ? h->st.warn.c_str() : "null handle"; }

int dvh_synchronize(dvh_handle* h) {
  if (!h) return DVH_ERR_ARG;
  DVH_HIP(h, hipStreamSynchronize(h->stream));
  return DVH_OK;
}

int dvh_last_host_syncs(const dvh_handle* h, int32_t* out) {
  if (!h || !out) return DVH_ERR_ARG;
  *out = h->n_syncs;
  return DVH_OK;
}

int dvh_last_certify(const dvh_handle* h, int32_t* out5) {
  if (!h || !out5) return DVH_ERR_ARG;
  for (int i = 0; i < 5; ++i) out5[i] = h->st.cert[i];
  return DVH_OK;
}

int dvh_last_certify_early(const dvh_handle* h, int32_t* out2) {
  if (!h || !out2) return DVH_ERR_ARG;
  out2[0] = h->st.cert_early[0];
  out2[1] = h->st.cert_early[1];
  return DVH_OK;
}

int dvh_last_certify_ms(const dvh_handle* h, double* ms) {
  if (!h || !ms) return DVH_ERR_ARG;
  *ms = h->st.cert_ms;
  return DVH_OK;
}

int dvh_last_stats(const dvh_handle* h, int32_t* out4) {
  if (!h || !out4) return DVH_ERR_ARG;
  out4[0] = h->st.n_ell;
  out4[1] = h->st.n_generic;
  out4[2] = h->last_variant;
  out4[3] = h->kernel_path == 1 ? 1 : 0;
  return DVH_OK;
}

// {ELL, generic, large, band, chain}: the first `n` of them (the three exports differ only in how many they return)
static int path_counts(const dvh_handle* h, int32_t* out, int n) {
  if (!h || !out) return DVH_ERR_ARG;
  const int32_t all[5] = {h->st.n_ell, h->st.n_generic, h->st.n_large, h->st.n_band, h->st.n_chain};
  std::copy(all, all + n, out);
  return DVH_OK;
}
int dvh_last_path_counts(const dvh_handle* h, int32_t* out3) { return path_counts(h, out3, 3); }
int dvh_last_path_counts4(const dvh_handle* h, int32_t* out4) { return path_counts(h, out4, 4); }
int dvh_last_path_counts5(const dvh_handle* h, int32_t* out5) { return path_counts(h, out5, 5); }

int dvh_last_band_variant(const dvh_handle* h, int32_t* out) {
  if (!h || !out) return DVH_ERR_ARG;
  *out = h->last_band_variant;
  return DVH_OK;
}

int dvh_last_chain_aborts(const dvh_handle* h, int32_t* out) {
  if (!h || !out) return DVH_ERR_ARG;
  *out = h->st.n_chain_aborts;
  return DVH_OK;
}

int dvh_set_launch_order(dvh_handle* h, const int32_t* order, int32_t count) {
  if (!h || count < 0 || (count > 0 && !order)) return DVH_ERR_ARG;
  h->order.clear();
  if (count == 0) return DVH_OK;
  std::vector<char> seen(count, 0);  // a permutation of 0 .. count - 1 (the kernels index windows with it)
  for (int32_t i = 0; i < count; ++i) {
    const int32_t k = order[i];
    if (k < 0 || k >= count || seen[k]) return fail(h, DVH_ERR_ARG, "launch order is not a permutation of 0 .. count - 1");
    seen[k] = 1;
  }
  h->order.assign(order, order + count);
  return DVH_OK;
}

int dvh_set_kernel_path(dvh_handle* h, int mode) {
  if (!h || mode < 0 || mode > 7) return DVH_ERR_ARG;
  h->kernel_path = mode;
  for (dvh_handle* p : h->peers) p->kernel_path = mode;
  return DVH_OK;
}

int dvh_last_timing(const dvh_handle* h, double* ms3) {
  if (!h || !ms3) return DVH_ERR_ARG;
  for (int i = 0; i < 3; ++i) ms3[i] = h->st.timing[i];
  return DVH_OK;
}

}  // extern "C"
