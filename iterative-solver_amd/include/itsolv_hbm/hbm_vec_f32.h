// hbm::VecF32: an HBM-resident vector STORED in binary32, for the Q space of a solve.
//
// The Q space is written once (a converted copy of an R vector, or a combination of older Q vectors)
// and afterwards only read -- by the gemm_inner / gemm_outer passes that dominate an iteration -- so
// held in f32 it takes half the HBM and half the bytes of every pass over it.  The logical element
// type stays double (value_type), so subspace matrices stay Matrix<double> and every kernel computes
// in FP64 on the widened values (include/subspace_hip.h "mixed precision"): an element is rounded
// once, to nearest-even, when it is stored.  A value beyond the binary32 range becomes +/-inf: vectors
// held in f32 must be scaled to its range (the solvers' Q vectors are normalised).
//
// Same shard layout as hbm::Vec (size, local_size, offset, compatible: the two are compatible with each
// other when their distributions agree).  It owns its block and deep-copies; it has no copy-on-write
// sharing, no deferred scale and no deferred fill -- none of which a write-once vector needs.
#pragma once
#include <memory>
#include <stdexcept>
#include <utility>
#include <vector>

#include "hbm_vec.h"

namespace molpro::linalg::hbm {

class VecF32 {
 public:
  using value_type = double;   //!< the logical element type; storage_type is what HBM holds
  using storage_type = float;

  VecF32() = default;
  VecF32(std::shared_ptr<Device> dev, size_t n_global) : m_dev(std::move(dev)), m_size(n_global) {
    auto [off, n] = m_dev->shard(n_global);
    m_offset = off;
    m_local = n;
    check_status(ssp_alloc_f32(m_dev->ctx(), m_local, &m_p), "ssp_alloc_f32");
  }
  //! A deep copy (one f32 -> f32 pass).
  VecF32(const VecF32& o) : m_dev(o.m_dev), m_size(o.m_size), m_local(o.m_local), m_offset(o.m_offset) {
    if (!o.m_p) return;
    check_status(ssp_alloc_f32(m_dev->ctx(), m_local, &m_p), "ssp_alloc_f32");
    const int s = ssp_mx_copy(m_dev->ctx(), m_p, SSP_F32, o.m_p, SSP_F32, 1.0, m_local);
    if (s != SSP_OK) {
      release();
      check_status(s, "ssp_mx_copy");
    }
  }
  VecF32(VecF32&& o) noexcept { swap(o); }
  VecF32& operator=(const VecF32& o) {
    if (this != &o) {
      VecF32 t(o);
      swap(t);
    }
    return *this;
  }
  VecF32& operator=(VecF32&& o) noexcept {
    VecF32 t(std::move(o));
    swap(t);
    return *this;
  }
  ~VecF32() { release(); }
  void swap(VecF32& o) noexcept {
    std::swap(m_dev, o.m_dev);
    std::swap(m_p, o.m_p);
    std::swap(m_size, o.m_size);
    std::swap(m_local, o.m_local);
    std::swap(m_offset, o.m_offset);
  }
  //! A vector of the same length and distribution whose contents are not initialised.
  VecF32 alloc_like() const { return VecF32(m_dev, m_size); }

  size_t size() const { return m_size; }
  size_t local_size() const { return m_local; }
  size_t offset() const { return m_offset; }
  const float* data() const { return m_p; }
  float* data() { return m_p; }
  ssp_ctx* ctx() const { return m_dev->ctx(); }
  const std::shared_ptr<Device>& device() const { return m_dev; }
  //! Same global length and shard as o (a VecF32 or a Vec).
  template <class V>
  bool compatible(const V& o) const {
    return m_size == o.size() && m_offset == o.offset() && m_local == o.local_size();
  }

  //! The shard's values, widened.
  std::vector<double> local_values() const {
    std::vector<float> f(m_local);
    check_status(ssp_download_f32(ctx(), f.data(), m_p, m_local), "ssp_download_f32");
    return std::vector<double>(f.begin(), f.end());
  }
  //! Stores v rounded to nearest (on the host).
  void set_local_values(const std::vector<double>& v) {
    if (v.size() != m_local) throw std::invalid_argument("VecF32::set_local_values: wrong length");
    std::vector<float> f(v.size());
    for (size_t i = 0; i < v.size(); ++i) f[i] = float(v[i]);
    check_status(ssp_upload_f32(ctx(), m_p, f.data(), m_local), "ssp_upload_f32");
  }

 private:
  void release() {
    if (m_p) ssp_free_f32(m_dev->ctx(), m_p);
    m_p = nullptr;
  }

  std::shared_ptr<Device> m_dev;
  float* m_p = nullptr;
  size_t m_size = 0, m_local = 0, m_offset = 0;
};

}  // namespace molpro::linalg::hbm
