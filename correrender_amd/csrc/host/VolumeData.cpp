#include "VolumeData.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace crfhost {

float halfToFloat(uint16_t h) {
    const uint32_t sign = uint32_t(h & 0x8000u) << 16, exponent = (h >> 10) & 31u, mantissa = h & 0x3FFu;
    uint32_t bits;
    if (exponent == 0) {  // zero or denormal: mantissa * 2^-24, exact in float
        const float magnitude = float(mantissa) * 5.9604644775390625e-8f;
        std::memcpy(&bits, &magnitude, sizeof bits);
        bits |= sign;
    } else if (exponent == 31) {
        bits = sign | 0x7F800000u | (mantissa << 13);
    } else {
        bits = sign | ((exponent + 112u) << 23) | (mantissa << 13);
    }
    float f;
    std::memcpy(&f, &bits, sizeof f);
    return f;
}

uint16_t floatToHalf(float f) {
    uint32_t bits;
    std::memcpy(&bits, &f, sizeof bits);
    const uint16_t sign = uint16_t((bits >> 16) & 0x8000u);
    const uint32_t magnitude = bits & 0x7FFFFFFFu;
    if (magnitude > 0x7F800000u) return uint16_t(sign | 0x7E00u | ((magnitude >> 13) & 0x3FFu));  // NaN stays NaN
    if (magnitude >= 0x47800000u) return uint16_t(sign | 0x7C00u);                                // 65536 and above
    uint32_t kept, rest, half;
    if (magnitude >= 0x38800000u) {  // a half normal (2^-14 and above): rebias, drop 13 bits
        const uint32_t v = magnitude - (112u << 23);
        kept = v >> 13;
        rest = v & 0x1FFFu;
        half = 0x1000u;
    } else {  // a half denormal: multiples of 2^-24
        const uint32_t exponent = magnitude >> 23;
        if (exponent < 102u) return sign;  // below 2^-25: zero
        const uint32_t shift = 126u - exponent;  // 14..24
        const uint32_t m = (magnitude & 0x7FFFFFu) | 0x800000u;
        kept = m >> shift;
        rest = m & ((1u << shift) - 1u);
        half = 1u << (shift - 1u);
    }
    if (rest > half || (rest == half && (kept & 1u))) kept++;  // to nearest even; a carry moves up one binade (or to inf)
    return uint16_t(sign | kept);
}

HostCacheEntryType::HostCacheEntryType(size_t numEntries, ScalarDataFormat format, uint16_t* dataOwned)
    : numEntries(numEntries), scalarDataFormatNative(format) {
    if (format == ScalarDataFormat::SHORT) {
        dataShort = dataOwned;
    } else if (format == ScalarDataFormat::FLOAT16) {
        dataFloat16 = dataOwned;
    } else {
        delete[] dataOwned;
        throw CalculatorError("Error in HostCacheEntryType: 16-bit data is SHORT or FLOAT16.");
    }
}

HostCacheEntryType::~HostCacheEntryType() {
    delete[] dataFloat;
    delete[] dataByte;
    delete[] dataShort;
    delete[] dataFloat16;
}

const void* HostCacheEntryType::getDataNative() const {
    switch (scalarDataFormatNative) {
        case ScalarDataFormat::BYTE: return dataByte;
        case ScalarDataFormat::SHORT: return dataShort;
        case ScalarDataFormat::FLOAT16: return dataFloat16;
        default: return dataFloat;
    }
}

const float* HostCacheEntryType::getDataFloat() const {
    if (!dataFloat) {
        auto* converted = new float[numEntries];
        for (size_t i = 0; i < numEntries; i++) converted[i] = getDataFloatAt(i);
        dataFloat = converted;
    }
    return dataFloat;
}

float HostCacheEntryType::getDataFloatAt(size_t idx) const {
    if (dataFloat) return dataFloat[idx];
    if (scalarDataFormatNative == ScalarDataFormat::BYTE) return float(dataByte[idx]) / 255.0f;
    if (scalarDataFormatNative == ScalarDataFormat::SHORT) return float(dataShort[idx]) / 65535.0f;
    if (scalarDataFormatNative == ScalarDataFormat::FLOAT16) return halfToFloat(dataFloat16[idx]);
    return 0.0f;
}

void HostCacheEntryType::switchNativeFormat(ScalarDataFormat newNativeFormat) {
    if (scalarDataFormatNative != ScalarDataFormat::FLOAT || newNativeFormat != ScalarDataFormat::FLOAT16)
        throw CalculatorError("Error in HostCacheEntryType::switchNativeFormat: "
                              "Currently, only switching from float to float16 is supported.");
    scalarDataFormatNative = newNativeFormat;
    dataFloat16 = new uint16_t[numEntries];
    for (size_t i = 0; i < numEntries; i++) dataFloat16[i] = floatToHalf(dataFloat[i]);
}

void VolumeData::setGridExtent(float dx, float dy, float dz) {
    box.min = {0.0f, 0.0f, 0.0f};
    box.max = {float(xs - 1) * dx, float(ys - 1) * dy, float(zs - 1) * dz};
    const float maxDimension = std::max(box.max[0], std::max(box.max[1], box.max[2]));
    for (int i = 0; i < 3; i++) {
        const float normalizedDimension = box.max[i] / maxDimension;
        boxRendering.min[i] = -normalizedDimension * 0.25f;
        boxRendering.max[i] = normalizedDimension * 0.25f;
    }
}

void VolumeData::setFieldData(const std::string& fieldName, int timeStepIdx, int ensembleIdx, const float* values) {
    const size_t n = getSlice3dEntryCount();
    auto* copy = new float[n];
    std::memcpy(copy, values, n * sizeof(float));
    storage[Access(fieldName, timeStepIdx, ensembleIdx)] = std::make_shared<HostCacheEntryType>(n, copy);
    if (std::find(fieldNames.begin(), fieldNames.end(), fieldName) == fieldNames.end()) fieldNames.push_back(fieldName);
    fieldMinMaxCache.clear();
    hostFieldCache.clear();
    dataGeneration++;
}

void VolumeData::setFieldData(const std::string& fieldName, int timeStepIdx, int ensembleIdx, ScalarDataFormat format,
                              const void* values) {
    if (format == ScalarDataFormat::FLOAT) return setFieldData(fieldName, timeStepIdx, ensembleIdx, static_cast<const float*>(values));
    const size_t n = getSlice3dEntryCount();
    HostCacheEntry entry;
    if (format == ScalarDataFormat::BYTE) {
        auto* copy = new uint8_t[n];
        std::memcpy(copy, values, n);
        entry = std::make_shared<HostCacheEntryType>(n, copy);
    } else {
        auto* copy = new uint16_t[n];
        std::memcpy(copy, values, n * sizeof(uint16_t));
        entry = std::make_shared<HostCacheEntryType>(n, format, copy);
    }
    storage[Access(fieldName, timeStepIdx, ensembleIdx)] = entry;
    if (std::find(fieldNames.begin(), fieldNames.end(), fieldName) == fieldNames.end()) fieldNames.push_back(fieldName);
    fieldMinMaxCache.clear();
    hostFieldCache.clear();
    dataGeneration++;
}

std::vector<std::string> VolumeData::getFieldNames(FieldType) const {
    std::vector<std::string> names = fieldNames;
    for (const auto& c : calculators) names.push_back(c->getOutputFieldName());
    return names;
}

HostCacheEntry VolumeData::getFieldEntryCpu(FieldType, const std::string& fieldName, int timeStepIdx, int ensembleIdx) {
    if (timeStepIdx < 0) timeStepIdx = 0;
    if (ensembleIdx < 0) ensembleIdx = 0;
    const Access access(fieldName, timeStepIdx, ensembleIdx);
    auto itCalc = calculatorsHost.find(fieldName);
    if (itCalc == calculatorsHost.end()) {
        auto it = storage.find(access);
        if (it == storage.end())
            throw CalculatorError("Error in VolumeData::getFieldEntryCpu: Trying to access field '" + fieldName +
                                  "' that is not available.");
        return it->second;
    }
    auto itCache = hostFieldCache.find(access);
    if (itCache != hostFieldCache.end()) return itCache->second;
    const size_t numEntries = getSlice3dEntryCount();
    auto* buffer = new float[numEntries];  // VolumeData.cpp:1222
    try {
        itCalc->second->calculateCpu(timeStepIdx, ensembleIdx, buffer);
    } catch (...) {
        delete[] buffer;
        throw;
    }
    HostCacheEntry entry = std::make_shared<HostCacheEntryType>(numEntries, buffer);  // takes ownership, :1226
    hostFieldCache[access] = entry;
    return entry;
}

std::pair<float, float> VolumeData::getMinMaxScalarFieldValue(const std::string& fieldName, int timeStepIdx,
                                                              int ensembleIdx) {
    if (timeStepIdx < 0) timeStepIdx = 0;
    if (ensembleIdx < 0) ensembleIdx = 0;
    auto itCalc = calculatorsHost.find(fieldName);
    if (itCalc != calculatorsHost.end() && itCalc->second->getHasFixedRange()) return itCalc->second->getFixedRange();
    const Access access(fieldName, timeStepIdx, ensembleIdx);
    auto it = fieldMinMaxCache.find(access);
    if (it != fieldMinMaxCache.end()) return it->second;
    HostCacheEntry entry = getFieldEntryCpu(FieldType::SCALAR, fieldName, timeStepIdx, ensembleIdx);
    const float* v = entry->data<float>();
    float mn = std::numeric_limits<float>::max(), mx = std::numeric_limits<float>::lowest();
    for (size_t i = 0; i < entry->getNumEntries(); i++) {
        if (v[i] < mn) mn = v[i];
        if (v[i] > mx) mx = v[i];
    }
    // Is this a divergent scalar field? If yes, the range is centred at zero (VolumeData.cpp:1661-1666).
    if (getIsScalarFieldDivergent(fieldName)) {
        const float maxAbs = std::max(std::abs(mn), std::abs(mx));
        mn = -maxAbs;
        mx = maxAbs;
    }
    fieldMinMaxCache[access] = {mn, mx};
    return {mn, mx};
}

void VolumeData::addCalculator(const CalculatorPtr& calculator) {
    calculator->initialize();
    calculator->setCalculatorId(calculators.size());
    calculator->setVolumeData(this, true);
    calculators.push_back(calculator);
    // Every calculator of this stand-in fulfils calculateCpu (a HIP backend has no Vulkan image to fill, so it is
    // dispatched like FilterDevice::CPU calculators are: VolumeData.cpp:1055-1059,1214-1226).
    calculatorsHost[calculator->getOutputFieldName()] = calculator;
}

void VolumeData::updateCalculators() {
    for (auto& c : calculators) {
        const bool nameChanged = c->getHasNameChanged();
        if (c->getIsDirty() || nameChanged) {
            for (auto it = calculatorsHost.begin(); it != calculatorsHost.end();)
                it = (it->second == c) ? calculatorsHost.erase(it) : std::next(it);
            calculatorsHost[c->getOutputFieldName()] = c;
            hostFieldCache.clear();
        }
    }
}

}  // namespace crfhost
