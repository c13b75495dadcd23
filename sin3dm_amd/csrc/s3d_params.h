// s3d_params.h — the parameter registry of the handles that take a state_dict (s3d_unet, s3d_decoder, s3d_ae): one record and one
// body for <handle>_param_info / <handle>_set_param, and the plane names their parameter keys are built from.
#pragma once
#include "s3d_common.h"

namespace s3d {

static const char* kPlane[3] = {"xy", "xz", "yz"};

struct ParamSpec {
    std::string name;
    std::vector<int64_t> shape;
    size_t numel() const { size_t n = 1; for (auto d : shape) n *= size_t(d); return n; }
};
// <handle>_param_info: name / ndim / shape of entry i.  specs is null for a null handle; what is "", "decoder " or "ae "
inline int registry_param_info(const std::vector<ParamSpec>* specs, const char* what, int i, const char** name, int64_t* shape, int* ndim) {
    S3D_CHECK(specs && i >= 0 && i < int(specs->size()), S3D_ERR_INVALID, "%sparam_info: index %d out of range", what, i);
    const ParamSpec& sp = (*specs)[i];
    if (name) *name = sp.name.c_str();
    if (ndim) *ndim = int(sp.shape.size());
    if (shape) for (size_t k = 0; k < sp.shape.size(); ++k) shape[k] = sp.shape[k];
    return 0;
}
// <handle>_set_param: find the name, compare the shape, store into the host map (the caller drops its packed images)
inline int registry_set_param(const std::vector<ParamSpec>* specs, std::map<std::string, std::vector<float>>* host, const char* what, const char* name,
                     const float* data, const int64_t* shape, int ndim) {
    S3D_CHECK(specs && name && data && shape, S3D_ERR_INVALID, "%sset_param: null argument", what);
    for (const auto& sp : *specs) {
        if (sp.name != name) continue;
        bool ok = int(sp.shape.size()) == ndim;
        for (int k = 0; ok && k < ndim; ++k) ok = sp.shape[k] == shape[k];
        S3D_CHECK(ok, S3D_ERR_INVALID, "size mismatch for %s", name);
        (*host)[sp.name].assign(data, data + sp.numel());
        return 0;
    }
    set_error("unexpected key '%s' in %sstate_dict", name, what);
    return S3D_ERR_INVALID;
}

}  // namespace s3d
