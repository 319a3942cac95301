// sample_key.h -- the sampling key of include/gnnagg.h ("Neighbour sampling"), one text for the device kernels (sample.hip) and the host
// sampler (host_graph.cpp).  murmur3's 32-bit finalizer, all arithmetic uint32 with wrap-around; a bijection of p for a fixed seed.
// The weighted key below it is built from that key, a 257-entry table of log2 and one float32 division.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GNNAGG_HD __host__ __device__
#else
#define GNNAGG_HD
#endif

namespace gnnagg {

GNNAGG_HD static inline uint32_t sample_fmix(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// once per call
GNNAGG_HD static inline uint32_t sample_seed_mix(unsigned long long seed)
{
    return sample_fmix(sample_fmix((uint32_t)seed + 0x9E3779B9u) ^ (uint32_t)(seed >> 32));
}

// p: the edge's position in the full CSR
GNNAGG_HD static inline uint32_t sample_key(uint32_t p, uint32_t s) { return sample_fmix(sample_fmix(p ^ s) + s); }

// ---- weighted sampling (gnnagg.h "Weighted sampling"): Efraimidis-Spirakis keys E / w with E = -log2 of the uniform key, in integer
// arithmetic and ONE correctly rounded float32 division, so that the device, the host and the numpy restatement agree bit for bit.

// L[i] = round(2^26 . log2(1 + i/256)), i = 0 ... 256 (every value lies at least 0.0029 from a half-integer)
GNNAGG_HD static inline uint32_t sample_log2_q26(uint32_t i)
{
    static constexpr uint32_t kSampleLog2[257] = {
        0u, 377457u, 753448u, 1127985u, 1501079u, 1872740u, 2242980u, 2611809u, 2979239u, 3345280u, 3709941u, 4073235u,
        4435170u, 4795758u, 5155007u, 5512929u, 5869532u, 6224826u, 6578822u, 6931527u, 7282953u, 7633108u, 7982000u, 8329640u,
        8676036u, 9021198u, 9365133u, 9707850u, 10049359u, 10389667u, 10728784u, 11066717u, 11403474u, 11739064u, 12073495u, 12406774u,
        12738911u, 13069911u, 13399784u, 13728537u, 14056177u, 14382713u, 14708150u, 15032498u, 15355762u, 15677951u, 15999071u, 16319130u,
        16638134u, 16956090u, 17273006u, 17588887u, 17903742u, 18217575u, 18530395u, 18842207u, 19153019u, 19462835u, 19771664u, 20079510u,
        20386381u, 20692282u, 20997220u, 21301200u, 21604229u, 21906312u, 22207456u, 22507666u, 22806948u, 23105307u, 23402750u, 23699282u,
        23994909u, 24289635u, 24583468u, 24876411u, 25168470u, 25459651u, 25749959u, 26039399u, 26327977u, 26615696u, 26902564u, 27188583u,
        27473761u, 27758100u, 28041608u, 28324287u, 28606143u, 28887182u, 29167407u, 29446823u, 29725435u, 30003247u, 30280265u, 30556493u,
        30831934u, 31106594u, 31380477u, 31653588u, 31925930u, 32197508u, 32468327u, 32738390u, 33007703u, 33276268u, 33544090u, 33811173u,
        34077521u, 34343139u, 34608030u, 34872199u, 35135648u, 35398383u, 35660406u, 35921722u, 36182335u, 36442249u, 36701466u, 36959991u,
        37217828u, 37474980u, 37731450u, 37987243u, 38242363u, 38496811u, 38750593u, 39003711u, 39256169u, 39507970u, 39759119u, 40009617u,
        40259469u, 40508678u, 40757247u, 41005180u, 41252479u, 41499149u, 41745191u, 41990610u, 42235408u, 42479589u, 42723155u, 42966110u,
        43208457u, 43450199u, 43691339u, 43931880u, 44171825u, 44411176u, 44649938u, 44888111u, 45125701u, 45362709u, 45599138u, 45834991u,
        46070271u, 46304980u, 46539122u, 46772699u, 47005714u, 47238169u, 47470068u, 47701412u, 47932205u, 48162449u, 48392147u, 48621302u,
        48849915u, 49077989u, 49305528u, 49532533u, 49759007u, 49984953u, 50210372u, 50435268u, 50659643u, 50883499u, 51106838u, 51329664u,
        51551977u, 51773782u, 51995079u, 52215872u, 52436163u, 52655953u, 52875246u, 53094043u, 53312346u, 53530159u, 53747482u, 53964319u,
        54180672u, 54396542u, 54611931u, 54826843u, 55041278u, 55255240u, 55468730u, 55681750u, 55894303u, 56106390u, 56318013u, 56529175u,
        56739877u, 56950121u, 57159911u, 57369246u, 57578130u, 57786564u, 57994550u, 58202091u, 58409188u, 58615842u, 58822057u, 59027833u,
        59233172u, 59438077u, 59642550u, 59846591u, 60050204u, 60253389u, 60456148u, 60658484u, 60860398u, 61061891u, 61262966u, 61463625u,
        61663868u, 61863698u, 62063117u, 62262125u, 62460725u, 62658919u, 62856708u, 63054094u, 63251078u, 63447662u, 63643848u, 63839637u,
        64035030u, 64230031u, 64424639u, 64618857u, 64812686u, 65006128u, 65199184u, 65391856u, 65584145u, 65776054u, 65967582u, 66158732u,
        66349506u, 66539905u, 66729930u, 66919582u, 67108864u,
    };
    return kSampleLog2[i];
}

// E(u) = -log2((u + 1/2) / 2^32) in Q6.26, 3 ... 33 . 2^26: the mantissa of 2u + 1 looked up in L, linear between two entries
GNNAGG_HD static inline uint32_t sample_neg_log2(uint32_t u)
{
    const uint32_t b = u ? 32u - (uint32_t)__builtin_clz(u) : 0u;                        // bit length of u
    const uint32_t fr = (uint32_t)((2ull * u + 1ull) << (32u - b));                      // (2u + 1) / 2^b - 1 in Q32
    const uint32_t i = fr >> 24, r = (fr >> 8) & 0xFFFFu;
    const uint32_t l0 = sample_log2_q26(i), l1 = sample_log2_q26(i + 1u);
    const uint32_t lg = l0 + (uint32_t)(((uint64_t)(l1 - l0) * r) >> 16);
    return ((33u - b) << 26) - lg;
}

constexpr uint32_t kSampleIneligible = 0xFFFFFFFFu;

// the weighted key of an edge with uniform key u = sample_key(p, s) and weight w: the bits of float32(E(u)) / w (>= 0: uint32 order is
// float order; +Inf and denormal quotients are kept as they are), kSampleIneligible unless w > 0 (0, -0, negative, NaN)
GNNAGG_HD static inline uint32_t sample_wkey(uint32_t u, float w)
{
    if (!(w > 0.0f)) return kSampleIneligible;
    const float e = (float)sample_neg_log2(u);
#if defined(__HIP_DEVICE_COMPILE__)
    const float q = __fdiv_rn(e, w);
    return __float_as_uint(q);
#else
    const float q = e / w;
    uint32_t bits;
    __builtin_memcpy(&bits, &q, sizeof bits);
    return bits;
#endif
}

}  // namespace gnnagg
