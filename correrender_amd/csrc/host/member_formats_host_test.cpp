// Test driver for the native member formats of the host layer (VolumeData.hpp: ScalarDataFormat, HostCacheEntryType):
//   member_formats_host_test convert <floats.bin> <outdir>   CPU only.  Dumps the float view of every u8, u16 and f16
//       code (u8.bin, u16.bin, f16.bin) and the FLOAT16 storage switchNativeFormat makes of the floats in floats.bin
//       (half.bin, uint16 bit patterns); tests/test_member_formats_host.py compares them with numpy.
//   member_formats_host_test upload <in.bin> <outdir>        needs the GPU.  in.bin: int32 xs, ys, zs, cs, format
//       (crf_member_format), then cs volumes in that format.  Evaluates the Pearson field of the ensemble through a
//       CorrelationCalculator fed through setFieldData(format), dumps it (pearson.bin) and prints the format of the
//       members the calculator left resident on the device.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "CorrelationCalculator.hpp"
#include "VolumeData.hpp"

using namespace crfhost;

template <class T>
static void dump(const std::string& path, const T* v, size_t n) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v), std::streamsize(n * sizeof(T)));
    if (!f) throw std::runtime_error("cannot write " + path);
}

static std::vector<char> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error(std::string("cannot read ") + path);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond);   \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

static int testConvert(const char* floatsPath, const std::string& outDir) {
    {
        std::vector<uint8_t> codes(256);
        std::iota(codes.begin(), codes.end(), uint8_t(0));
        VolumeData vol(256, 1, 1, 1, 1);
        vol.setFieldData("data", 0, 0, ScalarDataFormat::BYTE, codes.data());
        HostCacheEntry entry = vol.getFieldEntryCpu(FieldType::SCALAR, "data", 0, 0);
        CHECK(entry->getScalarDataFormatNative() == ScalarDataFormat::BYTE);
        CHECK(static_cast<const uint8_t*>(entry->getDataNative())[200] == 200);
        CHECK(entry->getDataNative() != codes.data());       // copied
        CHECK(entry->dataAt<float>(51) == 51.0f / 255.0f);   // before the view exists
        dump(outDir + "/u8.bin", entry->data<float>(), 256);
        CHECK(entry->data<float>() == entry->data<float>());  // converted once
        const auto mm = vol.getMinMaxScalarFieldValue("data", 0, 0);
        CHECK(mm.first == 0.0f && mm.second == 1.0f);
    }
    std::vector<uint16_t> codes(65536);
    std::iota(codes.begin(), codes.end(), uint16_t(0));
    for (const bool half : {false, true}) {
        const ScalarDataFormat format = half ? ScalarDataFormat::FLOAT16 : ScalarDataFormat::SHORT;
        VolumeData vol(256, 16, 16, 1, 1);
        vol.setFieldData("data", 0, 0, format, codes.data());
        HostCacheEntry entry = vol.getFieldEntryCpu(FieldType::SCALAR, "data", 0, 0);
        CHECK(entry->getScalarDataFormatNative() == format && entry->getNumEntries() == 65536);
        CHECK(static_cast<const uint16_t*>(entry->getDataNative())[40000] == 40000);
        dump(outDir + (half ? "/f16.bin" : "/u16.bin"), entry->data<float>(), 65536);
    }
    {
        const std::vector<char> raw = slurp(floatsPath);
        const size_t n = raw.size() / sizeof(float);
        VolumeData vol(int(n), 1, 1, 1, 1);
        vol.setFieldData("data", 0, 0, reinterpret_cast<const float*>(raw.data()));
        HostCacheEntry entry = vol.getFieldEntryCpu(FieldType::SCALAR, "data", 0, 0);
        CHECK(entry->getScalarDataFormatNative() == ScalarDataFormat::FLOAT && entry->getDataNative() == entry->data<float>());
        const float* before = entry->data<float>();
        entry->switchNativeFormat(ScalarDataFormat::FLOAT16);
        CHECK(entry->getScalarDataFormatNative() == ScalarDataFormat::FLOAT16);
        CHECK(entry->data<float>() == before);  // the float view stays the original, unrounded data
        dump(outDir + "/half.bin", static_cast<const uint16_t*>(entry->getDataNative()), n);
        bool threw = false;
        try {
            entry->switchNativeFormat(ScalarDataFormat::FLOAT16);  // FLOAT -> FLOAT16 is the only switch
        } catch (const CalculatorError&) {
            threw = true;
        }
        CHECK(threw);
    }
    std::puts("CONVERT-OK");
    return 0;
}

static int testUpload(const char* inPath, const std::string& outDir) {
    const std::vector<char> raw = slurp(inPath);
    const int32_t* head = reinterpret_cast<const int32_t*>(raw.data());
    const int xs = head[0], ys = head[1], zs = head[2], cs = head[3], format = head[4];
    const ScalarDataFormat native = format == CRF_MEMBER_U8    ? ScalarDataFormat::BYTE
                                    : format == CRF_MEMBER_U16 ? ScalarDataFormat::SHORT
                                    : format == CRF_MEMBER_F16 ? ScalarDataFormat::FLOAT16
                                                               : ScalarDataFormat::FLOAT;
    const size_t n = size_t(xs) * ys * zs;
    const size_t element = format == CRF_MEMBER_U8 ? 1 : format == CRF_MEMBER_F32 ? 4 : 2;
    CHECK(raw.size() == 5 * sizeof(int32_t) + n * element * size_t(cs));
    auto vol = std::make_shared<VolumeData>(xs, ys, zs, 1, cs);
    for (int e = 0; e < cs; e++)
        vol->setFieldData("data", 0, e, native, raw.data() + 5 * sizeof(int32_t) + size_t(e) * n * element);
    auto calc = std::make_shared<CorrelationCalculator>(0);
    vol->addCalculator(calc);
    calc->setSettings(SettingsMap{{"correlation_measure_type", "pearson"}});
    vol->updateCalculators();
    HostCacheEntry entry = vol->getFieldEntryCpu(FieldType::SCALAR, calc->getOutputFieldName(), 0, 0);
    dump(outDir + "/pearson.bin", entry->data<float>(), n);
    std::printf("RESIDENT-FORMAT %d\n", calc->getResidentMemberFormat());
    std::puts("UPLOAD-OK");
    return 0;
}

int main(int argc, char** argv) {
    try {
        if (argc >= 4 && std::string(argv[1]) == "convert") return testConvert(argv[2], argv[3]);
        if (argc >= 4 && std::string(argv[1]) == "upload") return testUpload(argv[2], argv[3]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    std::fprintf(stderr, "usage: member_formats_host_test convert <floats.bin> <outdir> | upload <in.bin> <outdir>\n");
    return 64;
}
