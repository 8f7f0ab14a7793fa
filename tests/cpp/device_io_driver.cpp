// Test driver for search_dev of the host-side mirror (auncel_amd/csrc/host): IndexIVFFlat::search_dev and
// IndexIVFFlatSubset::search_dev against search() of the same object on the same queries.  The queries go to device memory with
// hipMalloc + hipMemcpy; the results are rows inside larger device buffers whose other rows hold a sentinel.  It runs on a bundle
// prepared by tests/test_gpu_device_io_paths.py and writes what came out to a second bundle.
// usage: device_io_driver <in.tb> <out.tb>
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../auncel_amd/csrc/host/AuxIndexStructures.h"
#include "../../auncel_amd/csrc/host/FaissException.h"
#include "../../auncel_amd/csrc/host/IndexFlat.h"
#include "../../auncel_amd/csrc/host/IndexIVFFlat.h"
#include "../../include/auncel_amd.h"
#include "../../oracle/tbundle.h"

using namespace faiss;
typedef Index::idx_t idx_t;

static const size_t GUARD = 3;  // sentinel rows on either side of the results
static const float SENT_D = 12345.5f;
static const idx_t SENT_I = -777;

static void hip_ok(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// search() and search_dev() of ix on the same rows -> <p>host_D / _I, <p>dev_D / _I, <p>guards_ok, <p>dev_io
template <class IX> static void put_both(tb::Bundle& out, const std::string& p, const IX& ix, amd_ivf* engine, const tb::Tensor& xq, size_t k) {
    const size_t nq = xq.dims[0], d = xq.dims[1], rows = nq + 2 * GUARD;
    std::vector<float> D(nq * k);
    std::vector<idx_t> I(nq * k);
    ix.search((idx_t)nq, xq.as<float>(), (idx_t)k, D.data(), I.data());
    out.put_f32(p + "host_D", {nq, k}, D.data());
    out.put_i64(p + "host_I", {nq, k}, I.data());

    float *d_x = nullptr, *d_D = nullptr;
    idx_t* d_I = nullptr;
    hip_ok(hipMalloc((void**)&d_x, nq * d * sizeof(float)), "hipMalloc x");
    hip_ok(hipMalloc((void**)&d_D, rows * k * sizeof(float)), "hipMalloc D");
    hip_ok(hipMalloc((void**)&d_I, rows * k * sizeof(idx_t)), "hipMalloc I");
    std::vector<float> bigD(rows * k, SENT_D);
    std::vector<idx_t> bigI(rows * k, SENT_I);
    hip_ok(hipMemcpy(d_x, xq.as<float>(), nq * d * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy x");
    hip_ok(hipMemcpy(d_D, bigD.data(), bigD.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy D");
    hip_ok(hipMemcpy(d_I, bigI.data(), bigI.size() * sizeof(idx_t), hipMemcpyHostToDevice), "hipMemcpy I");
    ix.search_dev((idx_t)nq, d_x, (idx_t)k, d_D + GUARD * k, d_I + GUARD * k);
    uint64_t io[4] = {9, 9, 9, 9};
    amd_ivf_last_dev_io(engine, io);
    hip_ok(hipMemcpy(bigD.data(), d_D, bigD.size() * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy D back");
    hip_ok(hipMemcpy(bigI.data(), d_I, bigI.size() * sizeof(idx_t), hipMemcpyDeviceToHost), "hipMemcpy I back");
    hip_ok(hipFree(d_x), "hipFree");
    hip_ok(hipFree(d_D), "hipFree");
    hip_ok(hipFree(d_I), "hipFree");
    int64_t guards_ok = 1;
    for (size_t r = 0; r < rows; r++) {
        if (r >= GUARD && r < GUARD + nq) continue;
        for (size_t j = 0; j < k; j++) guards_ok &= bigD[r * k + j] == SENT_D && bigI[r * k + j] == SENT_I;
    }
    out.put_f32(p + "dev_D", {nq, k}, bigD.data() + GUARD * k);
    out.put_i64(p + "dev_I", {nq, k}, bigI.data() + GUARD * k);
    out.put_scalar_i64(p + "guards_ok", guards_ok);
    out.put_u64(p + "dev_io", {4}, io);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    try {
        tb::Bundle in = tb::Bundle::load(argv[1]), out;
        const size_t d = in.scalar<size_t>("d"), nlist = in.scalar<size_t>("nlist"), k = in.scalar<size_t>("k");
        const MetricType mt = in.scalar<int>("metric") == 0 ? METRIC_INNER_PRODUCT : METRIC_L2;
        const tb::Tensor &cen = in.get("centroids"), &xb = in.get("xb"), &xq = in.get("xq");
        IndexFlat q(d, mt);
        q.add(nlist, cen.as<float>());
        q.coarse_mode = 0;
        IndexIVFFlat ix(&q, d, nlist, mt);
        ix.is_trained = true;
        ix.coarse_mode = 0;
        ix.nprobe = in.scalar<size_t>("nprobe");
        ix.add(xb.dims[0], xb.as<float>());
        put_both(out, "flat_", ix, ix.engine(), xq, k);

        IndexIVFFlatSubset sub(ix, 0, in.scalar<int64_t>("range_lo"), in.scalar<int64_t>("range_hi"));  // (copy_subset_to type 0: an id range)
        sub.nprobe = ix.nprobe;
        sub.coarse_mode = 0;
        put_both(out, "subset_", sub, sub.engine(), xq, k);
        out.put_scalar_i64("subset_ntotal", sub.ntotal);
        out.save(argv[2]);
        printf("DONE\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION: %s\n", e.what());
        return 3;
    }
}
