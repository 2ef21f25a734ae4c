// VolumeData.hpp -- minimal host-side stand-in for the reference's field registry
// (/root/reference/src/Volume/VolumeData.hpp:95-483, VolumeData.cpp), reproducing only the contract the correlation
// calculators depend on:
//   grid / ensemble getters                       VolumeData.hpp:167-171
//   getFieldEntryCpu(type, name, t, e)            VolumeData.cpp:1202-1226: input fields come from storage; a field
//       whose name belongs to a host calculator is produced by allocating `new float[xs*ys*zs]`, calling
//       calc->calculateCpu(t, e, buffer) and wrapping the buffer in a HostCacheEntry that later delete[]s it
//       (Cache/HostCacheEntry.hpp:39-50) -- the callee must neither retain nor free the buffer;
//   getMinMaxScalarFieldValue(name, t, e)         VolumeData.cpp:1632-1670 (per (field,t,e) extrema, cached);
//       -- symmetrised to +-max|.| for a field flagged divergent (getIsScalarFieldDivergent, :616-621, :1661-1666);
//   getBoundingBoxRendering()                     VolumeData.hpp:205, computed by setGridExtent (VolumeData.cpp:322-330):
//       the world-space box picking positions are expressed in (ICorrelationCalculator::setReferencePointFromWorld);
//   addCalculator                                  VolumeData.cpp:1046-1086 (initialize, id, setVolumeData(this,true),
//       registered under getOutputFieldName()).
// No loaders, no device caches, no rendering: inputs are handed in as arrays.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "Calculator.hpp"

namespace crfhost {

/// Native storage format of a scalar field (the reference's ScalarDataFormat, src/Volume/Cache/HostCacheEntry.hpp).
enum class ScalarDataFormat { FLOAT, BYTE, SHORT, FLOAT16 };

/// IEEE binary16 <-> binary32 on the bit patterns: halfToFloat is exact (half denormals are float normals),
/// floatToHalf rounds to nearest even, overflows to infinity and keeps NaN a NaN (the reference's HalfFloat).
float halfToFloat(uint16_t h);
uint16_t floatToHalf(float f);

/// A field as it is stored (the reference's HostCacheEntryType, Cache/HostCacheEntry.cpp): the native array is kept and
/// the float view the calculators read is converted on first use -- b / 255.0f, s / 65535.0f, float(h)
/// (HostCacheEntry.cpp:107-176).
class HostCacheEntryType {
public:
    HostCacheEntryType(size_t numEntries, float* dataOwned) : numEntries(numEntries), dataFloat(dataOwned) {}
    HostCacheEntryType(size_t numEntries, uint8_t* dataOwned)
        : numEntries(numEntries), scalarDataFormatNative(ScalarDataFormat::BYTE), dataByte(dataOwned) {}
    /// 16-bit storage: format is SHORT (unsigned 16 bit) or FLOAT16 (binary16 bit patterns).
    HostCacheEntryType(size_t numEntries, ScalarDataFormat format, uint16_t* dataOwned);
    ~HostCacheEntryType();
    HostCacheEntryType(const HostCacheEntryType&) = delete;
    HostCacheEntryType& operator=(const HostCacheEntryType&) = delete;
    /// The float view (T = float is the only view the calculators use).
    template <class T>
    const T* data() const { return reinterpret_cast<const T*>(getDataFloat()); }
    template <class T>
    T dataAt(size_t idx) const { return T(getDataFloatAt(idx)); }
    size_t getNumEntries() const { return numEntries; }
    ScalarDataFormat getScalarDataFormatNative() const { return scalarDataFormatNative; }
    const void* getDataNative() const;
    const float* getDataFloat() const;
    float getDataFloatAt(size_t idx) const;
    /// FLOAT -> FLOAT16 only, as in the reference (HostCacheEntry.cpp:72-84); the float view stays as it is.
    void switchNativeFormat(ScalarDataFormat newNativeFormat);

private:
    size_t numEntries;
    ScalarDataFormat scalarDataFormatNative = ScalarDataFormat::FLOAT;
    mutable float* dataFloat = nullptr;  // the native array of FLOAT, else the lazily converted view
    uint8_t* dataByte = nullptr;
    uint16_t* dataShort = nullptr;
    uint16_t* dataFloat16 = nullptr;
};
typedef std::shared_ptr<HostCacheEntryType> HostCacheEntry;

/// Axis-aligned box with float corners (the two members of sgl::AABB3 the path reads).
struct AABB3 {
    std::array<float, 3> min{0.f, 0.f, 0.f}, max{0.f, 0.f, 0.f};
};

class VolumeData {
public:
    VolumeData(int xs, int ys, int zs, int ts, int es) : xs(xs), ys(ys), zs(zs), ts(ts), es(es) { setGridExtent(1.f, 1.f, 1.f); }

    /// Cell spacing -> box = [0, (n-1) d] and the rendering box: the box's dimensions divided by the largest one,
    /// times -+0.25 (VolumeData::setGridExtent, VolumeData.cpp:322-330).
    void setGridExtent(float dx, float dy, float dz);
    const AABB3& getBoundingBoxRendering() const { return boxRendering; }
    /// VolumeData.cpp:616-621: only the field named "Helicity" is centred at zero.
    bool getIsScalarFieldDivergent(const std::string& fieldName) const { return fieldName == "Helicity"; }

    int getGridSizeX() const { return xs; }
    int getGridSizeY() const { return ys; }
    int getGridSizeZ() const { return zs; }
    int getTimeStepCount() const { return ts; }
    int getEnsembleMemberCount() const { return es; }
    size_t getSlice3dEntryCount() const { return size_t(xs) * size_t(ys) * size_t(zs); }
    int getStandardScalarFieldIdx() const { return 0; }

    /// Registers the data of one (field, time step, ensemble member): xs*ys*zs floats, copied.
    void setFieldData(const std::string& fieldName, int timeStepIdx, int ensembleIdx, const float* values);
    /// The same for data in a native format: xs*ys*zs elements of `format` (uint8_t, uint16_t or binary16 bit patterns),
    /// copied and kept as they are; calculators see the converted float view, the device receives the native array.
    void setFieldData(const std::string& fieldName, int timeStepIdx, int ensembleIdx, ScalarDataFormat format,
                      const void* values);
    std::vector<std::string> getFieldNames(FieldType) const;

    HostCacheEntry getFieldEntryCpu(FieldType fieldType, const std::string& fieldName, int timeStepIdx = -1,
                                    int ensembleIdx = -1);
    std::pair<float, float> getMinMaxScalarFieldValue(const std::string& fieldName, int timeStepIdx = -1,
                                                      int ensembleIdx = -1);
    void addCalculator(const CalculatorPtr& calculator);
    /// Evicts the cached outputs of dirty calculators (the role of VolumeData::renderGuiCalculators, :1852-1936).
    void updateCalculators();
    size_t getNewCalculatorUseCount(CalculatorType t) { return ++calculatorTypeUseCounts[t]; }  // VolumeData.cpp:2283-2285
    /// Monotonic id of the input data (changes whenever setFieldData is called): lets a calculator keep a device copy.
    uint64_t getDataGeneration() const { return dataGeneration; }

private:
    typedef std::tuple<std::string, int, int> Access;
    int xs, ys, zs, ts, es;
    AABB3 box, boxRendering;
    std::vector<std::string> fieldNames;
    std::map<Access, HostCacheEntry> storage;         // input fields
    std::map<Access, HostCacheEntry> hostFieldCache;  // calculator outputs
    std::map<Access, std::pair<float, float>> fieldMinMaxCache;
    std::map<std::string, CalculatorPtr> calculatorsHost;
    std::vector<CalculatorPtr> calculators;
    std::map<CalculatorType, size_t> calculatorTypeUseCounts;
    uint64_t dataGeneration = 0;
};

}  // namespace crfhost
