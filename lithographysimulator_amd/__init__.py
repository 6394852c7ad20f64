"""MI355X-native Abbe aerial-image engine behind the object API of
quarterwave0/LithographySimulator (Mask / LightSource / Pupil / abbeImage)."""
from .imageformation import (PlanCache, abbeImage, abbeIntensity, bossungCurves, calculateFFTAerial,   # noqa: F401
                             embeddedSize, measureCD, postProcess, resistContour)
from ._native import engineOptions                                                      # noqa: F401
from .layout import (GdsLibrary, composeTransmission, flattenLayout, maskFromGDSII,       # noqa: F401
                     rasterizeLayout, readGDSII, writeGDSII)
from .lightsource import (LightSource, sourceShifts, sourceShiftsAsync, sourceWeights,   # noqa: F401
                          sourceWeightsAsync)
from .metrology import (LayoutSites, OPCResult, biasLayout, correctLayout,             # noqa: F401
                        imageRegistration, layoutSites, measureEPE)
from .contours import (Contours, contourVertices, contoursToGDSII, contoursToLayout,   # noqa: F401
                       doseFocusEnvelope, processVariationBand, simplifyContour, traceContours)
from .socs import (SOCSKernels, hopkinsImage, hopkinsIntensity, hopkinsIntensityBatch,  # noqa: F401
                   socsKernels)
from .tiling import (TiledImage, TilePlan, cutTiles, hopkinsImageTiled, maskImageTiled, maskPolygons,   # noqa: F401
                     optimizeMaskTiled, overlapAddTiles, planTiles, stitchTiles, tileValidRegion, unstitchTiles,
                     tileEdgeIndex, rasterizeLayoutTiles, correctLayoutTiled, epeJacobianTiled)
from .ilt import (ILTResult, bakedResistModel, developedResistModel, hopkinsFields,     # noqa: F401
                  hopkinsGradient, hopkinsGradientBatch, hopkinsIntensityAD, maskSpectrumAdjoint, optimizeMask, postProcessAdjoint)
from .smo import (SourceResult, optimizeSource, optimizeSourceMask, projectedStep,      # noqa: F401
                  sourceGradient, sourceLossGradient, sourceSensitivities)
from .aberrations import (AberrationResult, aberrationGradient, fitAberrations,         # noqa: F401
                          pupilGradient, wavefrontGradient, zernikeBasis)
from .vector import (sourcePolarization, vectorAbbeIntensity, vectorPupils,            # noqa: F401
                     vectorSocsKernels)
from .film import FilmStack, filmPupils                                                 # noqa: F401
from .develop import (MackResist, ResistProfile, developedDepth, developmentRate,      # noqa: F401
                      developmentRateGradient, developmentTime, developmentTimeGradient,
                      latentDiffusion, resistProfile, resistProfileGradient)
from .peb import (BakeResult, ChemicallyAmplifiedResist, amplifiedRateGradient,        # noqa: F401
                  bakeGradient, exposeAcidGradient, postExposureBake, postExposureBakeGradient)
from .calibrate import (bakeParameterChain, bakeParameterGradient, bakeStepGradient,  # noqa: F401
                        calibrateResist, exposureParameterGradient, rateParameterChain,
                        rateParameterGradient, resistArrivalTimes, resistParameter,
                        resistParameterGradient, resistWith)
from .tangent import (amplifiedRateTangent, bakeParameterTangent, bakeTangent,         # noqa: F401
                      calibrationJacobian, developmentRateTangent, developmentTimeTangent,
                      exposeAcidTangent, rateParameterTangent, resistProfileTangent)
from .sensitivity import (edgeCoverageTangent, epeJacobian, hopkinsTangent,            # noqa: F401
                          maskErrorFactor, measureCDTangent, measureEPETangent, postProcessTangent)
from .mask import Mask, alternatingPSM, attenuatedPSM                                   # noqa: F401
from .pupil import (OSAindexToMN, Pupil, generatePhi, generateWavefrontError,           # noqa: F401
                    generateZ, throughFocusPupils)

__all__ = ["Mask", "attenuatedPSM", "alternatingPSM", "LightSource", "Pupil", "abbeImage", "abbeIntensity", "calculateFFTAerial", "postProcess", "resistContour", "measureCD", "bossungCurves", "PlanCache", "engineOptions", "embeddedSize",
           "sourceShifts", "sourceShiftsAsync", "sourceWeights", "sourceWeightsAsync", "OSAindexToMN", "generateWavefrontError", "generatePhi", "generateZ",
           "throughFocusPupils", "readGDSII", "writeGDSII", "flattenLayout", "rasterizeLayout", "composeTransmission", "maskFromGDSII", "GdsLibrary",
           "imageRegistration", "layoutSites", "measureEPE", "biasLayout", "correctLayout", "LayoutSites", "OPCResult",
           "Contours", "contourVertices", "traceContours", "contoursToLayout", "simplifyContour", "contoursToGDSII", "doseFocusEnvelope",
           "processVariationBand", "SOCSKernels", "socsKernels", "hopkinsIntensity", "hopkinsImage",
           "hopkinsFields", "hopkinsGradient", "hopkinsIntensityAD", "maskSpectrumAdjoint", "postProcessAdjoint", "optimizeMask", "ILTResult",
           "sourceSensitivities", "sourceGradient", "sourceLossGradient", "projectedStep", "optimizeSource", "optimizeSourceMask",
           "SourceResult",
           "pupilGradient", "wavefrontGradient", "zernikeBasis", "aberrationGradient", "fitAberrations", "AberrationResult",
           "vectorPupils", "sourcePolarization", "vectorSocsKernels", "vectorAbbeIntensity",
           "FilmStack", "filmPupils",
           "MackResist", "ResistProfile", "latentDiffusion", "developmentRate", "developmentTime", "developedDepth", "resistProfile",
           "ChemicallyAmplifiedResist", "BakeResult", "postExposureBake",
           "bakeGradient", "exposeAcidGradient", "postExposureBakeGradient", "bakedResistModel",
           "developmentTimeGradient", "developmentRateGradient", "resistProfileGradient", "amplifiedRateGradient", "developedResistModel",
           "bakeStepGradient", "bakeParameterChain", "bakeParameterGradient", "rateParameterChain", "rateParameterGradient",
           "exposureParameterGradient", "resistParameterGradient", "calibrateResist", "resistArrivalTimes", "resistWith", "resistParameter",
           "exposeAcidTangent", "bakeTangent", "bakeParameterTangent", "developmentRateTangent", "amplifiedRateTangent",
           "rateParameterTangent", "developmentTimeTangent", "resistProfileTangent", "calibrationJacobian",
           "hopkinsTangent", "postProcessTangent", "edgeCoverageTangent", "measureEPETangent", "measureCDTangent", "epeJacobian",
           "maskErrorFactor",
           "hopkinsIntensityBatch", "tileValidRegion", "planTiles", "hopkinsImageTiled", "TilePlan", "TiledImage",
           "hopkinsGradientBatch", "cutTiles", "overlapAddTiles", "stitchTiles", "unstitchTiles", "optimizeMaskTiled", "maskPolygons", "maskImageTiled",
           "tileEdgeIndex", "rasterizeLayoutTiles", "correctLayoutTiled", "epeJacobianTiled"]
