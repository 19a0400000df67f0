// f3ds_ref_shim.h -- the slice of PCL, Eigen, Boost and OpenCV that the reference's merge half and scorer use (its clustering, clustering_state,
// testing and color_utilities sources), written from scratch so that those four files compile UNCHANGED on a machine that has none of the
// libraries.  TEST INFRASTRUCTURE ONLY (oracle/Makefile target `ref`, oracle/ref_driver.cpp); nothing in the product includes it.
//
// What is ours here and what is not:
//   * containers, point structs, PointCloud, Supervoxel, Matrix / Array: plain C++ with the semantics the reference relies on
//     (iteration order, push_back, operator+, first maximum of maxCoeff, column copies).
//   * vector arithmetic (dot, cross, norm, normalize): sequential float code in the summation order oracle/f3ds_oracle.cpp states for
//     Eigen 3.3 (sum3 = a + (b + c); a 4-vector sums (a + b) + (c + d); normalize divides by sqrt(squaredNorm) when that is > 0).
//   * the numerical primitives that belong to PCL and OpenCV -- computeCentroid, computePointNormal (eigen33), flipNormalTowardsViewpoint,
//     cvtColor(RGB2Lab) -- are NOT written again: they forward to the oracle's exports (f3ds_oracle_*), so they stay as unpinned as they
//     were.  What this build pins is the control flow and the float expressions of the reference's own four files.
//   * GlasbeyLUT is csrc/f3ds_glasbey.h, the project's own table (fence F4 of the oracle): colours are not compared.
//   * console::print_debug is ours: it keeps the three values Clustering::cluster hands it before every merge (survivor, absorbed, weight).
#ifndef F3DS_REF_SHIM_H_
#define F3DS_REF_SHIM_H_

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <iterator>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

extern "C" {
void f3ds_oracle_plane_params(const float* xyz, size_t n, float* plane4, float* curvature);
void f3ds_oracle_flip_normal(const float* point3, float vp_x, float vp_y, float vp_z, float* normal4);
void f3ds_oracle_centroid(const float* xyz, size_t n, float* centroid3);
void f3ds_oracle_unit_rgb2lab(const float* unit_rgb, float* lab);
}

// ---- boost ---------------------------------------------------------------------------------------------------------------------------
namespace boost {
template <class T> using shared_ptr = std::shared_ptr<T>;
template <class T, class... A> shared_ptr<T> make_shared(A&&... a) { return std::make_shared<T>(std::forward<A>(a)...); }
}  // namespace boost

// ---- Eigen ---------------------------------------------------------------------------------------------------------------------------
namespace Eigen {
const int Dynamic = -1;
template <class T> struct aligned_allocator : std::allocator<T> {
    template <class U> struct rebind { typedef aligned_allocator<U> other; };
    aligned_allocator() {}
    template <class U> aligned_allocator(const aligned_allocator<U>&) {}
};

struct Vector3f {
    float v[3];
    Vector3f() : v{0, 0, 0} {}
    Vector3f(float x, float y, float z) : v{x, y, z} {}
    float& operator[](int i) { return v[i]; }
    float operator[](int i) const { return v[i]; }
    Vector3f operator-(const Vector3f& o) const { return Vector3f(v[0] - o.v[0], v[1] - o.v[1], v[2] - o.v[2]); }
    Vector3f& operator/=(float s) { v[0] /= s; v[1] /= s; v[2] /= s; return *this; }
    float dot(const Vector3f& o) const { return v[0] * o.v[0] + (v[1] * o.v[1] + v[2] * o.v[2]); }
    float norm() const { return std::sqrt(dot(*this)); }
    Vector3f cross(const Vector3f& o) const { return Vector3f(v[1] * o.v[2] - v[2] * o.v[1], v[2] * o.v[0] - v[0] * o.v[2], v[0] * o.v[1] - v[1] * o.v[0]); }
};
struct Vector4f {
    float v[4];
    Vector4f() : v{0, 0, 0, 0} {}
    float& operator[](int i) { return v[i]; }
    float operator[](int i) const { return v[i]; }
    float squaredNorm() const { return (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]); }
    void normalize() {
        float z = squaredNorm();
        if (z > 0.0f) { float s = std::sqrt(z); v[0] /= s; v[1] /= s; v[2] /= s; v[3] /= s; }
    }
};

// dense storage of run-time size, column major; Rows / Cols only tell the types apart
template <class T, int Rows, int Cols> struct Array {
    size_t r = 0, c = 0;
    std::vector<T> d;
    Array() {}
    Array(size_t rows, size_t cols, T fill) : r(rows), c(cols), d(rows * cols, fill) {}
    static Array Zero(size_t rows, size_t cols) { return Array(rows, cols, T(0)); }
    T& operator()(size_t i) { return d[i]; }
    const T& operator()(size_t i) const { return d[i]; }
    Array operator-(T s) const { Array o(*this); for (T& x : o.d) x = x - s; return o; }
    template <class S> Array<bool, Rows, Cols> operator==(S s) const {
        Array<bool, Rows, Cols> o(r, c, false);
        for (size_t i = 0; i < d.size(); ++i) o.d[i] = (d[i] == (T)s);
        return o;
    }
    bool any() const { for (size_t i = 0; i < d.size(); ++i) if (d[i]) return true; return false; }
};
template <class T, int Rows, int Cols> struct Matrix {
    size_t r = 0, c = 0;
    std::vector<T> d;
    Matrix() {}
    Matrix(size_t rows, size_t cols, T fill) : r(rows), c(cols), d(rows * cols, fill) {}
    static Matrix Zero(size_t rows, size_t cols) { return Matrix(rows, cols, T(0)); }
    T& operator()(size_t i, size_t j) { return d[j * r + i]; }
    const T& operator()(size_t i, size_t j) const { return d[j * r + i]; }
    T& operator()(size_t i) { return d[i]; }
    const T& operator()(size_t i) const { return d[i]; }
    Matrix<T, Dynamic, 1> col(size_t j) const {      // (a copy: the reference assigns it to a vector of its own before it writes to it)
        Matrix<T, Dynamic, 1> o(r, 1, T(0));
        for (size_t i = 0; i < r; ++i) o.d[i] = d[j * r + i];
        return o;
    }
    // the first of the largest coefficients (Eigen's visitor replaces its candidate only by a strictly greater value)
    template <class I> T maxCoeff(I* index) const {
        size_t best = 0;
        for (size_t i = 1; i < d.size(); ++i) if (d[i] > d[best]) best = i;
        *index = (I)best;
        return d[best];
    }
    Array<T, Rows, Cols> array() const { Array<T, Rows, Cols> o(r, c, T(0)); o.d = d; return o; }
};
}  // namespace Eigen

// ---- pcl -----------------------------------------------------------------------------------------------------------------------------
namespace pcl {
struct RGB { uint8_t b, g, r, a; };
struct Normal {
    float normal_x = 0, normal_y = 0, normal_z = 0, curvature = 0;
    Eigen::Vector3f getNormalVector3fMap() const { return Eigen::Vector3f(normal_x, normal_y, normal_z); }
};
// f3ds_index rides in what is padding in PCL's 32-byte point: the reference copies points whole, so a voxel keeps the row it came from
struct PointXYZRGBA {
    float x = 0, y = 0, z = 0;
    uint8_t b = 0, g = 0, r = 0, a = 255;
    uint32_t f3ds_index = 0;
    Eigen::Vector3f getVector3fMap() const { return Eigen::Vector3f(x, y, z); }
};
struct PointXYZL { float x = 0, y = 0, z = 0; uint32_t label = 0; };
struct PointXYZRGBL {
    float x = 0, y = 0, z = 0;
    union { struct { uint8_t b, g, r, a; }; float rgb; uint32_t rgba; };
    uint32_t label = 0;
    PointXYZRGBL() : rgba(0xFF000000u) {}
};

template <class PointT> struct PointCloud {
    typedef std::vector<PointT, Eigen::aligned_allocator<PointT> > VectorType;
    typedef boost::shared_ptr<PointCloud<PointT> > Ptr;
    typedef boost::shared_ptr<const PointCloud<PointT> > ConstPtr;
    typedef typename VectorType::iterator iterator;
    typedef typename VectorType::const_iterator const_iterator;
    VectorType points;
    iterator begin() { return points.begin(); }
    iterator end() { return points.end(); }
    const_iterator begin() const { return points.begin(); }
    const_iterator end() const { return points.end(); }
    size_t size() const { return points.size(); }
    bool empty() const { return points.empty(); }
    void push_back(const PointT& p) { points.push_back(p); }
    PointCloud& operator+=(const PointCloud& o) { points.insert(points.end(), o.points.begin(), o.points.end()); return *this; }
    PointCloud operator+(const PointCloud& o) const { PointCloud out(*this); out += o; return out; }
};

template <class PointT> struct Supervoxel {
    typedef boost::shared_ptr<Supervoxel<PointT> > Ptr;
    Supervoxel() : voxels_(new PointCloud<PointT>()), normals_(new PointCloud<Normal>()) {}
    Normal normal_;
    PointXYZRGBA centroid_;
    typename PointCloud<PointT>::Ptr voxels_;
    typename PointCloud<Normal>::Ptr normals_;
};

namespace shim {
template <class PointT> std::vector<float> xyz_of(const PointCloud<PointT>& cloud) {
    std::vector<float> xyz(3 * cloud.size());
    size_t k = 0;
    for (const PointT& p : cloud.points) { xyz[k++] = p.x; xyz[k++] = p.y; xyz[k++] = p.z; }
    return xyz;
}
inline void copy_fields(const PointXYZL& a, PointXYZRGBL& b) { b.x = a.x; b.y = a.y; b.z = a.z; b.label = a.label; }
inline void copy_fields(const PointXYZRGBL& a, PointXYZL& b) { b.x = a.x; b.y = a.y; b.z = a.z; b.label = a.label; }
inline void copy_fields(const PointXYZRGBL& a, PointXYZRGBA& b) { b.x = a.x; b.y = a.y; b.z = a.z; b.b = a.b; b.g = a.g; b.r = a.r; b.a = a.a; }
inline void copy_fields(const PointXYZRGBA& a, PointXYZRGBL& b) { b.x = a.x; b.y = a.y; b.z = a.z; b.b = a.b; b.g = a.g; b.r = a.r; b.a = a.a; }
}  // namespace shim

template <class PointT> void computeCentroid(const PointCloud<PointT>& cloud, PointT& centroid) {
    std::vector<float> xyz = shim::xyz_of(cloud);
    float c[3];
    f3ds_oracle_centroid(xyz.data(), cloud.size(), c);
    centroid.x = c[0]; centroid.y = c[1]; centroid.z = c[2];
}
template <class PointT> bool computePointNormal(const PointCloud<PointT>& cloud, Eigen::Vector4f& plane_parameters, float& curvature) {
    std::vector<float> xyz = shim::xyz_of(cloud);
    f3ds_oracle_plane_params(xyz.data(), cloud.size(), plane_parameters.v, &curvature);
    return cloud.size() >= 3;
}
template <class PointT> void flipNormalTowardsViewpoint(const PointT& point, float vp_x, float vp_y, float vp_z, Eigen::Vector4f& normal) {
    const float p[3] = {point.x, point.y, point.z};
    f3ds_oracle_flip_normal(p, vp_x, vp_y, vp_z, normal.v);
}
template <class In, class Out> void copyPointCloud(const PointCloud<In>& in, PointCloud<Out>& out) {
    out.points.clear();
    for (const In& p : in.points) { Out q; shim::copy_fields(p, q); out.points.push_back(q); }
}

struct GlasbeyLUT {
    static RGB at(unsigned int color_id);
    static size_t size() { return 256; }
};

namespace console {
void print_debug(const char* format, ...);
void print_info(const char* format, ...);
void print_warn(const char* format, ...);
}  // namespace console
}  // namespace pcl

// ---- OpenCV --------------------------------------------------------------------------------------------------------------------------
#define CV_32FC3 21
namespace cv {
enum { COLOR_RGB2Lab = 45, COLOR_Lab2RGB = 57 };
struct Scalar {
    double val[4];
    Scalar(double a = 0, double b = 0, double c = 0, double d = 0) : val{a, b, c, d} {}
};
struct Vec3f {
    float val[3];
    float& operator[](int i) { return val[i]; }
    float operator[](int i) const { return val[i]; }
};
// one CV_32FC3 pixel is all the reference ever holds
struct Mat {
    Vec3f px;
    Mat(int rows, int cols, int type, const Scalar& s) {
        if (rows != 1 || cols != 1 || type != CV_32FC3) throw std::logic_error("ref_shim cv::Mat: only one CV_32FC3 pixel");
        px.val[0] = (float)s.val[0]; px.val[1] = (float)s.val[1]; px.val[2] = (float)s.val[2];
    }
    template <class T> T& at(int, int) { return px; }
};
inline void cvtColor(const Mat& src, Mat& dst, int code) {
    if (code != COLOR_RGB2Lab) throw std::logic_error("ref_shim cv::cvtColor: only COLOR_RGB2Lab is forwarded to the oracle");
    f3ds_oracle_unit_rgb2lab(src.px.val, dst.px.val);
}
}  // namespace cv

#endif  // F3DS_REF_SHIM_H_
