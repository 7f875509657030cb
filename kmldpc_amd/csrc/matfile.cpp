// matfile.cpp — kml_kmeans_dump_mat: the MAT-file writer.  Host only: no HIP,
// no context.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kmldpc_amd.h"

// ---- MAT-file level 5 writer (KMeans::DumpToMat, src/kmeans.cc:99-109) ----
// What lab::Mat does through matio (lib/lab/src/mat.cc): Mat_CreateVer(...,
// MAT_FT_DEFAULT) = a level-5 file, each variable written uncompressed
// (MAT_COMPRESSION_NONE) as an n x 1 column: WriteVector(complex) ->
// mxDOUBLE_CLASS with the complex flag (real part, then imaginary part),
// WriteVector(int32) -> mxINT32_CLASS, WriteComplex -> a 1 x 1 complex double.
namespace {
struct MatOut {
  std::string buf;
  void raw(const void *p, size_t n) { buf.append(static_cast<const char *>(p), n); }
  void u32(uint32_t v) { raw(&v, 4); }
  void pad8() {
    while (buf.size() % 8) buf.push_back('\0');
  }
  // one data element: tag (type, bytes) + data, padded to 8 bytes
  void element(uint32_t type, const void *p, size_t n) {
    u32(type);
    u32((uint32_t)n);
    raw(p, n);
    pad8();
  }
  enum { miINT8 = 1, miINT32 = 5, miUINT32 = 6, miDOUBLE = 9, miMATRIX = 14 };
  enum { mxDOUBLE_CLASS = 6, mxINT32_CLASS = 12 };
  void matrix(const char *name, uint32_t cls, bool cplx, int rows, const void *re, const void *im, size_t elem) {
    MatOut body;
    const uint32_t flags[2] = {cls | (cplx ? 0x0800u : 0u), 0u};
    body.element(miUINT32, flags, sizeof(flags));
    const int32_t dims[2] = {rows, 1};
    body.element(miINT32, dims, sizeof(dims));
    body.element(miINT8, name, strlen(name));
    const uint32_t t = cls == mxINT32_CLASS ? miINT32 : miDOUBLE;
    body.element(t, re, (size_t)rows * elem);
    if (cplx) body.element(t, im, (size_t)rows * elem);
    u32(miMATRIX);
    u32((uint32_t)body.buf.size());
    raw(body.buf.data(), body.buf.size());
  }
  void complex_vec(const char *name, const double *z, int n) {  // z interleaved (re, im)
    std::vector<double> re(n), im(n);
    for (int i = 0; i < n; ++i) {
      re[i] = z[2 * i];
      im[i] = z[2 * i + 1];
    }
    matrix(name, mxDOUBLE_CLASS, true, n, re.data(), im.data(), sizeof(double));
  }
};
}  // namespace

int kml_kmeans_dump_mat(const char *path, const double *data, int S, const double *clusters, const int32_t *idx,
                        const double *constellations, int Kc, const double *append) {
  if (!path || !data || !clusters || !idx || !constellations || !append || S < 0 || Kc < 0) return KML_E_ARG;
  MatOut m;
  char hdr[128];
  memset(hdr, ' ', sizeof(hdr));
  const char *text = "MATLAB 5.0 MAT-file, Platform: GLNXA64, Created by: kmldpc_amd (KMeans::DumpToMat)";
  memcpy(hdr, text, strlen(text));
  memset(hdr + 116, 0, 8);  // subsystem data offset: none
  const uint16_t ver = 0x0100;
  memcpy(hdr + 124, &ver, 2);
  hdr[126] = 'I';  // written little-endian: reads back as "IM"
  hdr[127] = 'M';
  m.raw(hdr, sizeof(hdr));
  m.complex_vec("data", data, S);
  m.complex_vec("cluster", clusters, Kc);
  m.matrix("idx", MatOut::mxINT32_CLASS, false, S, idx, nullptr, sizeof(int32_t));
  m.complex_vec("constellations", constellations, Kc);
  m.complex_vec("hHats", append, 4);   // append[0..3]
  m.complex_vec("realH", append + 8, 1);  // append[4] (WriteComplex: 1 x 1)
  FILE *f = fopen(path, "wb");
  if (!f) return KML_E_IO;
  const bool ok = fwrite(m.buf.data(), 1, m.buf.size(), f) == m.buf.size();
  return (fclose(f) == 0 && ok) ? KML_OK : KML_E_IO;
}
